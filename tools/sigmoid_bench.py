"""The pairwise sigmoid loss call against the InfoNCE call, interleaved in one process, HIP events.

    python tools/sigmoid_bench.py [--reps 30] [--warmup 5] [--inner 10] [--out profiles/sigmoid_observed.txt]

Per shape (B, E, row0, nrows) -- (512, 512) and (4096, 512) in full and the last 512 rows of 4096 (one rank of eight) -- two variants on
the same L2-normalised random operands, both through the C ABI with every gradient requested (no host work beyond the call):
  sigmoid   vipant_sigmoid_loss_fwd_bwd: split / transpose, one walk, fold;
  infonce   vipant_infonce_fwd_bwd, the launch group of the `ce` head.
A repetition times `--inner` calls between two events and the variants take turns inside every repetition, so they see the same
clocks.  Per variant one JSON line: median, quartiles, min / max of the per-call milliseconds, the spread q75 - q25, the workspace,
and the MFMA operations the method needs over the median (sigmoid: two walks of 2 B n (3 E + E) multiply-adds each; InfoNCE:
6 B^2 E as bench.py counts it).  The register / LDS use of every kernel instantiation of csrc/sigmoid_loss.hip follows: registers and
static LDS as the build recorded them, the walk's dynamic LDS from the launcher's formula."""
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
    from vipant_amd import _ffi, build
    _ffi.call("vipant_device_check")
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    lines = []
    for B, E, row0, nrows in SHAPES:
        g = torch.Generator(device=dev).manual_seed(B + nrows)
        x1 = torch.nn.functional.normalize(torch.randn(B, E, generator=g, device=dev), dim=-1)
        x2 = torch.nn.functional.normalize(x1 + torch.randn(B, E, generator=g, device=dev) / E ** 0.5, dim=-1)
        par = torch.tensor([2.302585, -10.0, 2.659260], device=dev)       # log 10, the bias, log(1 / 0.07)
        out = torch.empty(8, device=dev)
        d1, d2 = torch.empty(nrows, E, device=dev), torch.empty(nrows, E, device=dev)
        nb_s = _ffi.query("vipant_sigmoid_loss_workspace_bytes", B, E, nrows)
        nb_n = _ffi.query("vipant_infonce_strip_workspace_bytes", B, E, nrows)
        ws_s, ws_n = (torch.empty(n, dtype=torch.uint8, device=dev) for n in (nb_s, nb_n))

        def sigmoid():
            _ffi.call("vipant_sigmoid_loss_fwd_bwd", x1.data_ptr(), x2.data_ptr(), par.data_ptr(), par.data_ptr() + 4, 0.0, out.data_ptr(),
                      d1.data_ptr(), d2.data_ptr(), out.data_ptr() + 4, out.data_ptr() + 8, 1.0, B, E, row0, nrows, ws_s.data_ptr(), nb_s, stream)

        def infonce():
            _ffi.call("vipant_infonce_fwd_bwd", x1.data_ptr(), x2.data_ptr(), par.data_ptr() + 8, 0.0, out.data_ptr() + 16, d1.data_ptr(),
                      d2.data_ptr(), out.data_ptr() + 20, 1.0, B, E, row0, nrows, ws_n.data_ptr(), nb_n, stream)

        times = interleaved((("sigmoid", sigmoid), ("infonce", infonce)), args.reps, args.warmup, args.inner)
        flops = {"sigmoid": 2 * 2.0 * B * nrows * 4 * E * 2, "infonce": 6.0 * B * B * E}
        for name, nb in (("sigmoid", nb_s), ("infonce", nb_n)):
            st = stats(times[name])
            lines.append(json.dumps(dict({"what": "loss call", "variant": name, "B": B, "E": E, "row0": row0, "nrows": nrows, "reps": args.reps,
                                          "inner": args.inner}, **st, spread_ms=round(st["q75_ms"] - st["q25_ms"], 4),
                                         workspace_mb=round(nb / 1e6, 2), method_tflops=round(flops[name] / (st["median_ms"] * 1e-3) / 1e12, 1))))
    for kernel, u in sorted(build.resource_usage().get("sigmoid_loss.hip", {}).items()):
        # the walk's LDS is dynamic: the queries' rows, then the waves' partial sums -- max(16 (4 E + 16), 8192 NCT) bytes at the widest E
        # instantiation NCT serves (64 NCT in one chunk up to NCT = 4, 128 NCT in two chunks from NCT = 5)
        nct = int(kernel.split("sig_walk_kernelILi")[1][0]) if "sig_walk_kernelILi" in kernel else 0
        dyn = max(16 * (4 * (64 if nct < 5 else 128) * nct + 16), 8192 * nct) if nct else 0
        lines.append(json.dumps({"what": "kernel resources", "kernel": kernel, "dynamic_lds_bytes_at_widest_E": dyn, "vgprs": u.get("VGPRs"), "agprs": u.get("AGPRs"),
                                 "spilled_vgprs": u.get("VGPRs Spill"), "scratch_bytes_per_lane": u.get("ScratchSize [bytes/lane]"),
                                 "static_lds_bytes": u.get("LDS Size [bytes/block]"), "waves_per_simd": u.get("Occupancy [waves/SIMD]")}))
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
