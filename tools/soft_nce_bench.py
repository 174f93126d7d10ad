"""The similarity-weighted InfoNCE call against the label-aware and the plain InfoNCE calls, interleaved in one process, HIP events.

    python tools/soft_nce_bench.py [--reps 30] [--warmup 5] [--inner 10] [--out profiles/soft_nce_observed.txt]

Per shape (B, E, row0, nrows) -- (512, 512) and (4096, 512) in full and the last 512 rows of 4096 (one rank of eight) -- four variants on
the same L2-normalised random operands, all through the autograd functions of vipant_amd.ops with every gradient requested (forward
only: the fused calls leave their gradients in the forward):
  soft_x2   ops.SoftNCEFn with t = x2 (the teacher product reads x2's own copies), w_floor = -1, w_power = 1;
  soft_t    ops.SoftNCEFn with a separate teacher [B, E];
  label     ops.LabelNCEFn, a third of the rows in one group, the rest spread over 100 (tools/label_nce_bench.py's ids);
  infonce   ops.InfoNCEFn, the launch group of the `ce` head.
A repetition times `--inner` calls between two events and the variants take turns inside every repetition, so they see the same
clocks.  Per variant one JSON line: median, quartiles, min / max of the per-call milliseconds, the spread q75 - q25, and the loss.  The
register / LDS use of every kernel instantiation of csrc/soft_nce.hip follows, as the build recorded it (the walks' LDS is dynamic: 64
KiB of stages, and in the gradient walk 128 bytes per column of a chunk)."""
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
        t = torch.nn.functional.normalize(x2.detach() + torch.randn(B, E, generator=g, device=dev) / E ** 0.5, dim=-1)
        draw = torch.rand(B, generator=g, device=dev)
        ids = torch.where(draw < 1.0 / 3.0, 0, 1 + torch.randint(0, 100, (B,), generator=g, device=dev)).to(torch.int32)
        ls = torch.tensor(2.659260, device=dev, requires_grad=True)       # log(1 / 0.07)
        out = {}

        def soft_x2():
            out["soft_x2"] = ops.SoftNCEFn.apply(x1, x2, x2.detach(), -1.0, 1.0, ls, 0.0, row0, nrows, 1.0)

        def soft_t():
            out["soft_t"] = ops.SoftNCEFn.apply(x1, x2, t, -1.0, 1.0, ls, 0.0, row0, nrows, 1.0)

        def label():
            out["label"] = ops.LabelNCEFn.apply(x1, x2, ids, ls, 0.0, row0, nrows, 1.0)

        def infonce():
            out["infonce"] = ops.InfoNCEFn.apply(x1, x2, ls, 0.0, row0, nrows, 1.0)

        variants = (("soft_x2", soft_x2), ("soft_t", soft_t), ("label", label), ("infonce", infonce))
        times = interleaved(variants, args.reps, args.warmup, args.inner)
        for name, _ in variants:
            st = stats(times[name])
            lines.append(json.dumps(dict({"what": "loss call", "variant": name, "B": B, "E": E, "row0": row0, "nrows": nrows,
                                          "reps": args.reps, "inner": args.inner}, **st,
                                         spread_ms=round(st["q75_ms"] - st["q25_ms"], 4), loss=round(float(out[name].detach()), 5))))
    for kernel, u in sorted(build.resource_usage().get("soft_nce.hip", {}).items()):
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
