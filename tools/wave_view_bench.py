"""Cost of the waveform views of the log-mel front-end, interleaved on one box, HIP events.

    python tools/wave_view_bench.py [--batch 512] [--reps 20] [--warmup 3] [--inner 2]

11-second 16 kHz clips (176000 samples; max_len 1000, so the pipeline crops to 160800) -> [b, 1, 1000, 128], norms and SpecAugment
masks on, fixed seeded draws:
  plain        vipant_fbank on input cropped beforehand ([b, 160800]: what a loader that crops would hand over);
  crop         vipant_fbank_view, the crop rule only (drawn windows);
  chain        vipant_fbank_view, RandomFlip(0.5) RandomScale(1.25) RandomPad(176000) RandomCrop(176000) RandomNoise(10, 120, 0.25),
               then the crop rule;
  chain_noisy  the same with RandomNoise(p = 1): every sample of every clip pays for its Philox block;
  unfused      the chain through vipant_wave_view (the transformed waveform written to a second buffer), then vipant_fbank;
  unfused_noisy  likewise for p = 1.
The fused and unfused routes must give the same bits before their times are compared (printed as `same_bits`).

tools/tagging_bench.py's method: a repetition times `--inner` calls between two events and the variants take turns inside every
repetition, so they see the same clocks.  Per variant one JSON line: median, quartiles, min / max of the per-call milliseconds."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.tagging_bench import interleaved, stats  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=2)
    args = ap.parse_args()
    from vipant_amd import _ffi
    from vipant_amd.frontend import KaldiFbank
    _ffi.call("vipant_device_check")
    dev = torch.device("cuda:0")
    sr, n, T, F, b = 16000, 176000, 1000, 128, args.batch
    kw = dict(norms=(-4.94, 5.76), freq_mask_param=32, time_mask_param=200, device=dev)
    chain = lambda p: [["RandomFlip", [0.5]], ["RandomScale", [1.25]], ["RandomPad", [n]], ["RandomCrop", [n]], ["RandomNoise", [10.0, 120.0, p]]]
    plain = KaldiFbank(sr, F, T, **kw)
    raw = KaldiFbank(sr, F, T, zero_mean_wf=False, **kw)                       # for a waveform whose mean is already gone
    fbs = {"chain": KaldiFbank(sr, F, T, audio_transforms=chain(0.25), **kw), "chain_noisy": KaldiFbank(sr, F, T, audio_transforms=chain(1.0), **kw)}
    g = torch.Generator().manual_seed(b)
    t = torch.arange(n) / sr
    wave = (0.05 * torch.randn(b, n, generator=g) + 0.1 * torch.sin(2 * torch.pi * 440.0 * t)).to(dev)
    cropped = wave[:, :plain.crop_len].contiguous()
    masks = plain.draw_masks(b, g).to(dev)
    crop_view = plain.draw_views(b, g)
    views = {k: fb.draw_views(b, torch.Generator().manual_seed(7)) for k, fb in fbs.items()}

    def unfused(k):
        w, m = fbs[k].view_wave(wave, None, views[k])
        return raw(w, m, masks)
    variants = [("plain", lambda: plain(cropped, None, masks)), ("crop", lambda: plain(wave, None, masks, view=crop_view))]
    for k in fbs:
        variants.append((k, lambda k=k: fbs[k](wave, None, masks, view=views[k])))
        variants.append(("unfused" + k[5:], lambda k=k: unfused(k)))
    same = {k: bool(torch.equal(fbs[k](wave, None, masks, view=views[k]), unfused(k))) for k in fbs}
    times = interleaved(variants, args.reps, args.warmup, args.inner)
    for name, _ in variants:
        extra = {"same_bits": same[name]} if name in same else {}
        if name in views:
            extra["noisy_clips"] = int((views[name][0][:, 4] >= 0).sum())
        print(json.dumps(dict({"what": "wave view", "variant": name, "b": b, "samples": n, "reps": args.reps, "inner": args.inner},
                              **stats(times[name]), **extra)), flush=True)


if __name__ == "__main__":
    main()
