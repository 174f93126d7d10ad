"""Patchout at the headline audio shape, interleaved in one process, HIP events.

    python tools/patchout_bench.py [--batch 512] [--layers 12] [--reps 10] [--warmup 3] [--out profiles/patchout_observed.txt]

x fp32 [batch, 1, 1024, 128], patch 32 x 32, stride 16 x 24 (63 x 5 = 315 patches, 316 tokens), width 768, the channel-mean kernel.
(a) the operator alone, forward with the weight-gradient operand stored: ops.PatchoutEmbedFn at keep = P (every patch, through the list)
    against ops.PatchEmbedFn (im2col + vipant_gemm_nt_tokens), `--inner` calls between two events.
(b) one training step of the audio tower -- forward, read-out, backward to every parameter -- with patchout.keep in {1.0, 0.75, 0.5}
    against the same tower without the key, one step between two events.
The variants take turns inside every repetition, so they see the same clocks.  Per variant one JSON line: median, quartiles, min / max
milliseconds, the spread q75 - q25, and for (b) the tokens per clip and the time relative to the tower without the key.  The register
and LDS use of every kernel of csrc/patch_keep.hip follows, as the build recorded it."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tagging_bench import interleaved, stats  # noqa: E402

T, F, PATCH, STRIDE, WIDTH = 1024, 128, 32, (16, 24), 768


def build_head(layers, patchout):
    import vipant_amd.module as M
    from vipant_amd.config import compose
    cfg = compose((f"+running=bimodal +running/audio=default +model/image=vit_val +model/audio=vit_val +model/text=dummy "
                   f"model.image.width={WIDTH} model.image.encoder.layers={layers} model.image.pre_encoder.patch_size={PATCH} "
                   f"model.audio.pre_encoder.stride=[{STRIDE[0]},{STRIDE[1]}] model.audio.resolution=[{T},{F}] " +
                   ("+model.audio.pre_encoder.patchout.keep=1.0" if patchout else "")).split())
    return M.build_audio_head(cfg.model.audio)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from vipant_amd import _ffi, build, ops
    _ffi.call("vipant_device_check")
    dev = torch.device("cuda:0")
    b = args.batch
    nrow, ncol = (T - PATCH) // STRIDE[0] + 1, (F - PATCH) // STRIDE[1] + 1
    P = nrow * ncol
    g = torch.Generator().manual_seed(b)
    x = torch.randn(b, 1, T, F, generator=g).to(dev)
    gy = torch.randn(b, 512, generator=g).to(dev)
    torch.manual_seed(0)
    plain, po = build_head(args.layers, False).to(dev).train(), build_head(args.layers, True).to(dev).train()
    po.load_state_dict(plain.state_dict(), strict=True)
    lines = []

    # (a) the operator alone
    pre = plain.pre_encoder
    opargs = (x, pre.conv1.weight, plain.misc.cls_embedding, plain.misc.pos_embedding, pre.ln.weight, pre.ln.bias, tuple(pre.stride))
    every = ops.draw_patchout(b, nrow, ncol, keep=P).to(dev)
    variants = [("patch_embed", lambda: ops.PatchEmbedFn.apply(*opargs)), ("patchout_embed_keep_all", lambda: ops.PatchoutEmbedFn.apply(*opargs, every))]
    with torch.no_grad():       # the two contractions sum in different orders: the largest difference of the LayerNorm outputs
        diff = float((variants[0][1]() - variants[1][1]()).abs().max())
    times = interleaved(variants, args.reps, args.warmup, args.inner)
    for name, _ in variants:
        st = stats(times[name])
        lines.append(json.dumps(dict({"what": "operator forward", "variant": name, "batch": b, "patches": P, "width": WIDTH, "reps": args.reps,
                                      "inner": args.inner, "max_abs_diff_to_patch_embed": diff}, **st, spread_ms=round(st["q75_ms"] - st["q25_ms"], 4))))

    # (b) the tower's training step
    def step(head, frac):
        def run():
            if frac is not None:
                head.pre_encoder.patchout = {"keep": frac}
            for p in head.parameters():
                p.grad = None
            head(x, normalized=True).backward(gy)
        return run

    variants = [("tower", step(plain, None))] + [(f"tower_keep_{f}", step(po, f)) for f in (1.0, 0.75, 0.5)]
    times = interleaved(variants, args.reps, args.warmup, 1)
    base = stats(times["tower"])["median_ms"]
    for (name, _), frac in zip(variants, (None, 1.0, 0.75, 0.5)):
        st = stats(times[name])
        tokens = 1 + (P if frac is None else max(int(frac * P), 1))
        lines.append(json.dumps(dict({"what": "tower training step", "variant": name, "batch": b, "layers": args.layers, "tokens_per_clip": tokens,
                                      "token_fraction": round(tokens / (P + 1), 4), "time_fraction": round(st["median_ms"] / base, 4),
                                      "reps": args.reps}, **st, spread_ms=round(st["q75_ms"] - st["q25_ms"], 4))))
    for kernel, u in sorted(build.resource_usage().get("patch_keep.hip", {}).items()):
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
