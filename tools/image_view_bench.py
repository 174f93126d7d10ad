"""Timing of the image views at the training batch: 512 decoded 360 x 640 frames -> [512, 3, 224, 224], the `clip` chain and both
`barlow` views (vipant_amd/image_views.py), HIP events around 20 calls after a warm-up, three repetitions each, interleaved.
Appends to profiles/image_view_observed.txt.  Usage: python tools/image_view_bench.py [--out FILE]"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vipant_amd.image_views import ImageViews  # noqa: E402

dev = torch.device("cuda:0")
b, H, W, n, calls = 512, 360, 640, 224, 20
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "image_view_observed.txt")
g = torch.Generator().manual_seed(1)
frames = torch.randint(0, 256, (b, H, W, 3), generator=g, dtype=torch.uint8).to(dev)
chains = {"clip": ImageViews(n, "clip", device=dev), "barlow prime": ImageViews(n, "barlow", device=dev, which="prime"),
          "barlow second": ImageViews(n, "barlow", device=dev, which="second")}
draws = {k: (v.draw_image_views([[H, W]] * b, g) if v.chain == "barlow" else None) for k, v in chains.items()}
times = {k: [] for k in chains}
for k, v in chains.items():                                     # warm-up: code objects, the workspace
    v(frames, draws=draws[k])
torch.cuda.synchronize()
for rep in range(3):
    for k, v in chains.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            out = v(frames, draws=draws[k])
        e1.record()
        torch.cuda.synchronize()
        times[k].append(e0.elapsed_time(e1) / calls)
lines = [f"image views, b = {b}, {H} x {W} uint8 frames -> {n} x {n} fp32 ({torch.cuda.get_device_name(0)}); ms per batch, "
         f"{calls} calls per repetition, 3 interleaved repetitions (host draws not included)"]
for k, t in times.items():
    byt = frames.numel() + b * 3 * n * n * 4
    lines.append(f"  {k:14s} min {min(t):7.3f}  median {sorted(t)[1]:7.3f}  max {max(t):7.3f} ms   ({b / sorted(t)[1] * 1e3:9.0f} frames/s, "
                 f"{byt / sorted(t)[1] / 1e6:6.1f} GB/s of frames-in + views-out)")
text = "\n".join(lines)
print(text)
with open(out_path, "a") as f:
    f.write(text + "\n")
