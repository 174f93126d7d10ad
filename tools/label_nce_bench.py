"""The label-aware InfoNCE call against the InfoNCE and the pairwise sigmoid calls, interleaved in one process, HIP events.

    python tools/label_nce_bench.py [--reps 30] [--warmup 5] [--inner 10] [--out profiles/label_nce_observed.txt]

Per shape (B, E, row0, nrows) -- (512, 512) and (4096, 512) in full and the last 512 rows of 4096 (one rank of eight) -- three variants
on the same L2-normalised random operands, all through the autograd functions of vipant_amd.ops with every gradient requested (forward
only: the fused calls leave their gradients in the forward):
  label     ops.LabelNCEFn: split / transpose, the stats walk over all B rows, the gradient walk over the strip, fold; about a third of
            the rows share one group id, the rest are spread over 100 groups (AudioSet's "Speech" and the tail);
  infonce   ops.InfoNCEFn, the launch group of the `ce` head;
  sigmoid   ops.SigmoidLossFn, the launch group of the `sigmoid` head.
A repetition times `--inner` calls between two events and the variants take turns inside every repetition, so they see the same
clocks.  Per variant one JSON line: median, quartiles, min / max of the per-call milliseconds, the spread q75 - q25, and the loss (the
label variant's differs from InfoNCE's by its positives).  The register / LDS use of every kernel instantiation of csrc/label_nce.hip
follows, as the build recorded it (the walks' LDS is dynamic: 16 (4 E + 16) bytes of query rows, and in the gradient walk at least the
waves' partial sums, 8192 bytes per 64 columns of a chunk)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tagging_bench import interleaved, stats  # noqa: E402

SHAPES = ((512, 512, 0, 512), (4096, 512, 0, 4096), (4096, 512, 3584, 512))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from vipant_amd import _ffi, build, ops
    _ffi.call("vipant_device_check")
    dev = torch.device("cuda:0")
    lines = []
    for B, E, row0, nrows in SHAPES:
        g = torch.Generator(device=dev).manual_seed(B + nrows)
        x1 = torch.nn.functional.normalize(torch.randn(B, E, generator=g, device=dev), dim=-1).requires_grad_()
        x2 = torch.nn.functional.normalize(x1.detach() + torch.randn(B, E, generator=g, device=dev) / E ** 0.5, dim=-1).requires_grad_()
        draw = torch.rand(B, generator=g, device=dev)
        ids = torch.where(draw < 1.0 / 3.0, 0, 1 + torch.randint(0, 100, (B,), generator=g, device=dev)).to(torch.int32)
        ls, lb = (torch.tensor(v, device=dev, requires_grad=True) for v in (2.659260, -10.0))       # log(1 / 0.07), the sigmoid bias
        out = {}

        def label():
            out["label"] = ops.LabelNCEFn.apply(x1, x2, ids, ls, 0.0, row0, nrows, 1.0)

        def infonce():
            out["infonce"] = ops.InfoNCEFn.apply(x1, x2, ls, 0.0, row0, nrows, 1.0)

        def sigmoid():
            out["sigmoid"] = ops.SigmoidLossFn.apply(x1, x2, ls, lb, 0.0, row0, nrows, 1.0)

        times = interleaved((("label", label), ("infonce", infonce), ("sigmoid", sigmoid)), args.reps, args.warmup, args.inner)
        for name in ("label", "infonce", "sigmoid"):
            st = stats(times[name])
            lines.append(json.dumps(dict({"what": "loss call", "variant": name, "B": B, "E": E, "row0": row0, "nrows": nrows,
                                          "largest_group": int(ids.bincount().max()), "reps": args.reps, "inner": args.inner}, **st,
                                         spread_ms=round(st["q75_ms"] - st["q25_ms"], 4), loss=round(float(out[name].detach()), 5))))
    for kernel, u in sorted(build.resource_usage().get("label_nce.hip", {}).items()):
        lines.append(json.dumps({"what": "kernel resources", "kernel": kernel, "vgprs": u.get("VGPRs"), "agprs": u.get("AGPRs"),
                                 "spilled_vgprs": u.get("VGPRs Spill"), "scratch_bytes_per_lane": u.get("ScratchSize [bytes/lane]"),
                                 "static_lds_bytes": u.get("LDS Size [bytes/block]"), "waves_per_simd": u.get("Occupancy [waves/SIMD]")}))
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
