"""Can the file loader keep one GPU fed?  On a generated directory of 256 ten-second stereo 16 kHz WAVs and 360 x 640 JPEG frames
(the reference's layout, vipant_amd/data): clips per second of the loader alone -- decode + collate + the parent's hand-over, batches
of 32 over an index that names every file four times (1024 items) -- at `num_proc` 0, 4 and 12.  Workers are spawned, which takes
seconds per pass whatever its length, so the time to the first batch is reported apart and the rate is that of the batches after
it; two passes each.  Then the device time of `pcm_wave` at b = 64 and 512 (HIP events, 30 repetitions, median and spread).
Appends to profiles/src_loader_observed.txt.  Usage: python tools/src_loader_bench.py [--out FILE] [--no-gpu]"""
import json
import os
import sys
import tempfile
import time
import warnings
import wave

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vipant_amd.config import to_config  # noqa: E402
from vipant_amd.data import build_image_audio_dataloader  # noqa: E402

N, SECONDS, SR, H, W, BATCH, REPEAT = 256, 10, 16000, 360, 640, 32, 4


def generate(root):
    from PIL import Image
    g = np.random.default_rng(1)
    os.makedirs(f"{root}/clip"), os.makedirs(f"{root}/frame")
    yy, xx = np.mgrid[0:H, 0:W]
    for i in range(N):
        pcm = np.clip(np.rint(6000 * g.standard_normal((SECONDS * SR, 2))), -32768, 32767).astype("<i2")
        with wave.open(f"{root}/clip/v{i}.wav", "wb") as f:
            f.setnchannels(2), f.setsampwidth(2), f.setframerate(SR)
            f.writeframes(pcm.tobytes())
        # smooth colour fields with a little noise: JPEGs of about the size a video frame gives
        ph = g.uniform(0, 6.28, 3)
        img = np.stack([127 + 100 * np.sin(xx / (40.0 + 10 * c) + ph[c]) * np.cos(yy / (30.0 + 7 * c)) for c in range(3)], -1)
        img = np.clip(img + 8 * g.standard_normal(img.shape), 0, 255).astype(np.uint8)
        Image.fromarray(img).save(f"{root}/frame/v{i}.jpg", quality=90)
    with open(f"{root}/src_bench.csv", "w") as index:
        for i in range(REPEAT * N):
            index.write(json.dumps({"id": f"v{i % N}", "dir": "", "clip": ["wav"], "frame": "jpg", "labels": ["x"]}) + "\n")


def loader_rate(root, workers):
    cfg = to_config({"seed": 1213, "num_proc": workers, "running": {
        "data_root": root, "eval_samples": 10 ** 9, "train_samples": 1.0, "frame_key": "frame", "frame_emb": None, "resolution": 224,
        "embed_dim": 512, "sample_rate": SR, "batch_size": BATCH, "multi_view": False}})
    _, loader = build_image_audio_dataloader(cfg, "src_bench", shuffle=False, train=True)
    passes = []
    for _ in range(2):
        t0, t1, n = time.perf_counter(), None, 0
        for batch in loader:
            if t1 is None:
                t1 = time.perf_counter()          # the first batch: worker start-up is behind us
            else:
                n += len(batch[4])
        passes.append((t1 - t0, n / (time.perf_counter() - t1)))
    return passes


def kernel_times(b, reps=30):
    from vipant_amd.frontend import pcm_wave
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(2)
    pcm = torch.randint(-32768, 32768, (b, 2 * SECONDS * SR), generator=g, dtype=torch.int32).to(torch.int16).to(dev)
    nframes = torch.full((b,), SECONDS * SR, dtype=torch.int64, device=dev)
    channels = torch.full((b,), 2, dtype=torch.int32, device=dev)
    out = {}
    for mode in ("first", "mean"):
        for _ in range(3):
            pcm_wave(pcm, nframes, channels, mode=mode, wave_stride=SECONDS * SR)
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            pcm_wave(pcm, nframes, channels, mode=mode, wave_stride=SECONDS * SR)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        out[mode] = sorted(ts)
    return out


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "src_loader_observed.txt")
    lines = [f"file loader alone, {N} x {SECONDS} s stereo {SR} Hz WAV + {H} x {W} JPEG named {REPEAT} times, batches of {BATCH}, "
             f"OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', '-')}; per pass: seconds to the first batch, clips/s of the batches after it"]
    with tempfile.TemporaryDirectory() as root, warnings.catch_warnings():
        warnings.simplefilter("ignore")
        generate(root)
        for workers in (0, 4, 12):
            (s1, r1), (s2, r2) = loader_rate(root, workers)
            lines.append(f"  num_proc {workers:2d}: first batch after {s1:5.2f} / {s2:5.2f} s, then {r1:8.1f} / {r2:8.1f} clips/s")
            print(lines[-1], flush=True)
    if "--no-gpu" not in sys.argv:
        lines.append(f"pcm_wave, {SECONDS} s stereo clips -> fp32 mono ({torch.cuda.get_device_name(0)}); us per launch, HIP events, 30 "
                     "repetitions after 3 warm-up calls")
        for b in (64, 512):
            for mode, ts in kernel_times(b).items():
                byt = b * SECONDS * SR * (4 + 4)          # int16 stereo in, fp32 mono out
                lines.append(f"  b = {b:3d} {mode:5s}: min {ts[0]:7.1f}  median {ts[len(ts) // 2]:7.1f}  max {ts[-1]:7.1f} us   "
                             f"({byt / ts[len(ts) // 2] / 1e3:7.1f} GB/s of pcm-in + wave-out)")
    text = "\n".join(lines)
    print(text)
    with open(out_path, "a") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
