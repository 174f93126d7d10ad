"""Timing of the GPU log-mel front-end at the training batch: 512 clips x 10.05 s at 16 kHz -> [512, 1, 1000, 128].
Usage: python tools/fbank_bench.py
       python tools/fbank_bench.py --pair [--batches 64 512] [--reps 20] [--warmup 3] [--inner 2]

--pair: the two masked views of the siamese dataset, ten-second 16 kHz clips -> 2 x [b, 1, 1000, 128],
FbankTransform's constants, prime masks (32, 200) on view 1 and second masks (48, 300) on view 2, the same seeded draws:
  single  one vipant_fbank_view launch (view 1 alone: what a step without `model.loss.aa` pays);
  two     two vipant_fbank_view launches, one per view;
  pair    one vipant_fbank_view_pair launch.
`two` and `pair` must give the same bits before their times are compared (printed as `same_bits`).  tools/tagging_bench.py's
method: a repetition times `--inner` calls between two HIP events and the variants take turns inside every repetition, so they see
the same clocks.  Per variant one JSON line: median, quartiles, min / max of the per-call milliseconds."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vipant_amd.frontend import KaldiFbank  # noqa: E402

dev = "cuda:0"


def single():
    for sr, b in ((16000, 512), (44100, 512)):
        n = int(10.05 * sr)
        fb = KaldiFbank(sr, 128, 1000, norms=(-4.94, 5.76), freq_mask_param=32, time_mask_param=200, device=dev)
        w = 0.1 * torch.randn(b, n, device=dev)
        masks = fb.draw_masks(b).to(dev)
        fb(w, None, masks); torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            out = fb(w, None, masks)
        e1.record(); torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / 10
        byt = w.numel() * 4 + out.numel() * 4
        print(f"sr={sr} b={b}: {ms:7.3f} ms per batch  ({b / ms * 1e3:9.0f} clips/s, {byt / ms / 1e6:6.1f} GB/s of waveform-in + fbank-out)")


def pair(args):
    from tools.tagging_bench import interleaved, stats
    sr, n, T, F = 16000, 160000, 1000, 128
    fb = KaldiFbank(sr, F, T, norms=(-4.93839311, 5.75751113), device=dev)
    for b in args.batches:
        g = torch.Generator().manual_seed(b)
        t = torch.arange(n) / sr
        wave = (0.05 * torch.randn(b, n, generator=g) + 0.1 * torch.sin(2 * torch.pi * 440.0 * t)).to(dev)
        view = fb.draw_views(b, g)
        m1 = fb.draw_masks(b, g, freq_mask_param=32, time_mask_param=200).to(dev)
        m2 = fb.draw_masks(b, g, freq_mask_param=48, time_mask_param=300).to(dev)
        variants = [("single", lambda: fb(wave, None, m1, view=view)),
                    ("two", lambda: (fb(wave, None, m1, view=view), fb(wave, None, m2, view=view))),
                    ("pair", lambda: fb(wave, None, m1, view=view, masks2=m2, pair=True))]
        two, one = variants[1][1](), variants[2][1]()
        same = bool(torch.equal(two[0], one[0]) and torch.equal(two[1], one[1]))
        del two, one
        times = interleaved(variants, args.reps, args.warmup, args.inner)
        for name, _ in variants:
            print(json.dumps(dict({"what": "fbank pair", "variant": name, "b": b, "samples": n, "reps": args.reps, "inner": args.inner,
                                   "same_bits": same}, **stats(times[name]))), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--pair", action="store_true")
    ap.add_argument("--batches", nargs="+", type=int, default=[64, 512])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=2)
    args = ap.parse_args()
    if args.pair:
        pair(args)
    else:
        single()
