"""Cost of the tagging trainer's two new launches, interleaved on one box, HIP events.

    python tools/tagging_bench.py [--batches 64 512] [--reps 30] [--warmup 5] [--inner 4]

Front-end, 10-second 16 kHz clips -> [b, 1, 1000, 128], norms and SpecAugment masks on, mixup rate 0.5 (fixed seeded draws):
  fused   vipant_fbank_mix: the mix formed inside the log-mel launch (three launches);
  torch   the only composition without it: the mixed waveform made with torch ops in a second [b, n] buffer
          (zero-mean, gather the partners, lambda-blend, zero-mean again), then vipant_fbank;
  plain   vipant_fbank on the unmixed batch.
Loss head, (B, C) = (512, 527), forward + backward of BCELossHead through ops.ClassifierFn on binary and on soft targets.

A repetition times `--inner` calls between two events and the three (two) variants take turns inside every repetition, so they
see the same clocks.  Per variant: median, quartiles and min / max of the per-call milliseconds, one JSON line each; the bytes a
front-end call has to move (computed from the shapes) over its median time are given as GB/s."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def stats(v):
    v = sorted(v)
    q = lambda f: v[min(int(f * len(v)), len(v) - 1)]
    return {"median_ms": round(q(0.5), 4), "q25_ms": round(q(0.25), 4), "q75_ms": round(q(0.75), 4), "min_ms": round(v[0], 4),
            "max_ms": round(v[-1], 4)}


def interleaved(variants, reps, warmup, inner):
    times = {name: [] for name, _ in variants}
    for it in range(warmup + reps):
        for name, fn in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if it >= warmup:
                times[name].append(e0.elapsed_time(e1) / inner)
    return times


def torch_mix(wave, index, lam):
    """cvap/data/audioset_cls.py:374-398 for a batch of equal-length clips, with torch ops: a second [b, n] buffer."""
    c = wave - wave.mean(dim=1, keepdim=True)
    partner = torch.where(index < 0, torch.arange(wave.shape[0], device=wave.device), index.long())
    lam = lam.unsqueeze(1)
    mixed = lam * c + (1.0 - lam) * c[partner]
    return mixed - mixed.mean(dim=1, keepdim=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", nargs="+", type=int, default=[64, 512])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=4)
    args = ap.parse_args()
    import vipant_amd.module as M
    from vipant_amd import _ffi, ops
    from vipant_amd.config import to_config
    from vipant_amd.frontend import KaldiFbank
    _ffi.call("vipant_device_check")
    dev = torch.device("cuda:0")
    sr, n, T, F = 16000, 160000, 1000, 128
    for b in args.batches:
        fb = KaldiFbank(sr, F, T, norms=(-4.94, 5.76), freq_mask_param=32, time_mask_param=200, device=dev)
        g = torch.Generator().manual_seed(b)
        wave = (0.1 * torch.randn(b, n, generator=g)).to(dev)
        masks = fb.draw_masks(b, g).to(dev)
        index, lam = (t.to(dev) for t in fb.draw_mixup(b, 0.5, g))
        variants = (("fused", lambda: fb(wave, None, masks, mix=(index, lam))),
                    ("torch", lambda: fb(torch_mix(wave, index, lam), None, masks)),
                    ("plain", lambda: fb(wave, None, masks)))
        # same clips, same draws: the two mixing paths must agree before their times are compared
        diff = float((variants[0][1]() - variants[1][1]()).abs().max())
        times = interleaved(variants, args.reps, args.warmup, args.inner)
        nmixed = int((index >= 0).sum())
        # bytes a call must move at least: every clip read for its mean and for its frames' first touch (the overlap of frames
        # and the second mean pass hit L2 when a clip fits), partners once more, the output written
        need = {"fused": (b + nmixed) * n * 4 + b * T * F * 4, "plain": b * n * 4 + b * T * F * 4,
                "torch": b * n * 4 * 2 + b * n * 4 + b * T * F * 4}          # read + write the mixed buffer, read it again
        for name, _ in variants:
            st = stats(times[name])
            print(json.dumps(dict({"what": "frontend", "variant": name, "b": b, "mixed": nmixed, "reps": args.reps, "inner": args.inner},
                                  **st, min_GBps=round(need[name] / st["median_ms"] / 1e6, 1),
                                  **({"max_abs_diff_fused_vs_torch": diff} if name == "fused" else {}))), flush=True)
    B, C = 512, 527
    head = M.build_loss_head(to_config({"name": "BCELossHead", "embed_dim": 512, "width": 768, "layers": [], "scaling": True, "bias": False,
                                        "soft_targets": True}), output_dim=C).to(dev).train()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, 512, generator=g).to(dev).requires_grad_()
    hard = (torch.rand(B, C, generator=g) < 0.01).to(torch.uint8).to(dev)
    perm = torch.randperm(B, generator=g).to(dev)
    soft = 0.4 * hard.float() + 0.6 * hard.float()[perm]

    def step(y):
        def run():
            with torch.no_grad():
                head.linear[1].weight.add_(0.0)          # a new parameter version, as after an optimizer step: weights are re-cast
            head.zero_grad(set_to_none=True)
            head(x, y).backward(gradient=ops.unit_grad(dev))
        return run
    times = interleaved((("binary", step(hard)), ("soft", step(soft))), args.reps, args.warmup, args.inner)
    for name in ("binary", "soft"):
        print(json.dumps(dict({"what": "bce head fwd+bwd", "targets": name, "B": B, "C": C, "reps": args.reps, "inner": args.inner},
                              **stats(times[name]))), flush=True)


if __name__ == "__main__":
    main()
