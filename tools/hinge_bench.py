"""The multi-label hinge loss call against the BCE call, interleaved in one process, HIP events.

    python tools/hinge_bench.py [--reps 30] [--warmup 5] [--inner 20] [--out profiles/hinge_observed.txt]

At B = 512, C = 527 (a tagging batch of AudioSet; logits padded to 576 columns as ops.ClassifierFn hands them over), uint8 marks of 2.7
labels a clip, logit_scale = log(1 / 0.07): ops.hinge_logits and ops.bce_logits with the gradient, and both forward only with the
scores (what `infer` asks for).  A repetition times `--inner` calls between two events and the variants take turns inside every
repetition, so they see the same clocks.  Per variant one JSON line: median, quartiles, min / max of the per-call milliseconds, the
spread q75 - q25 and the loss.  Then the call's errors against nn.MultiLabelMarginLoss in float64 on the host (autograd gradients) at
B = 64 and one C per register depth of the kernel (64, 128, 256, 527, 1024, and 1100 for the rows it reads twice), scaled logits uniform
in [-8, 8] with one row at +-40: loss and dscale relative, the scores in ulp of fp32, dz in bf16 units of the float64 value rounded to
bf16 (less the 2^-53 s / B that float64 autograd itself loses where p has rounded to 1).  The register use of every kernel
instantiation of csrc/hinge.hip follows, as the build recorded it."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tagging_bench import interleaved, stats  # noqa: E402


def errors(ops, C, B=64):
    g = torch.Generator().manual_seed(C)
    ls = float(torch.tensor(2.659260))              # the fp32 value the kernel is handed: both sides exponentiate the same number
    s = float(torch.tensor(ls).double().exp())
    z = ((16 * torch.rand(B, C, generator=g) - 8) / s).float()
    z[0] = torch.where(torch.rand(C, generator=g) < 0.5, 40.0, -40.0) / s
    t = torch.rand(B, C, generator=g) < 0.3
    lab = torch.where(t, torch.arange(C).expand(B, C), C).sort(dim=1)[0]            # convert_label: the positives' ids, then -1
    zd, lsd = z.double().requires_grad_(), torch.tensor(ls, dtype=torch.float64, requires_grad=True)
    rp = torch.sigmoid(lsd.exp() * zd)
    rl = torch.nn.MultiLabelMarginLoss()(rp, torch.where(lab == C, -1, lab))
    rl.backward()
    rl = rl.detach()
    loss, dz, dls, prob = (v.cpu().double() for v in ops.hinge_logits(z.cuda(), t.to(torch.uint8).cuda(), torch.tensor(ls).cuda(),
                                                                       want_prob=True))
    rb, rp = zd.grad.float().bfloat16().double(), rp.detach()
    unit = lambda ref, bits: torch.ldexp(torch.ones_like(ref), torch.frexp(ref)[1] - bits)
    e_dz = ((dz - rb).abs() - 2.0 ** -53 * s / B).clamp_min(0)
    return {"what": "errors against float64", "B": B, "C": C, "loss_rel": float((loss - rl).abs() / rl), "dscale_rel": float((dls - lsd.grad).abs() / lsd.grad.abs()),
            "prob_ulp": round(float(((prob - rp).abs() / unit(rp, 24)).max()), 3), "dz_bf16_units": round(float((e_dz / unit(rb, 8))[rb != 0].max()), 3),
            "dz_where_ref_is_0": float(e_dz[rb == 0].max()) if (rb == 0).any() else 0.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from vipant_amd import _ffi, build, ops
    _ffi.call("vipant_device_check")
    dev = torch.device("cuda:0")
    B, C, Cp = 512, 527, 576
    g = torch.Generator(device=dev).manual_seed(B + C)
    z = 0.5 * torch.randn(B, Cp, generator=g, device=dev)
    t = (torch.rand(B, C, generator=g, device=dev) < 2.7 / C).to(torch.uint8)
    ls = torch.tensor(2.659260, device=dev)
    out = {}
    variants = []
    for name, fn in (("hinge", ops.hinge_logits), ("bce", ops.bce_logits)):
        def train(name=name, fn=fn):
            out[name] = fn(z, t, ls, C=C, ldd=Cp)[0]

        def infer(name=name, fn=fn):
            out[name + "_infer"] = fn(z, t, ls, C=C, want_grad=False, want_prob=True)[0]

        variants += [(name, train), (name + "_infer", infer)]
    times = interleaved(variants, args.reps, args.warmup, args.inner)
    lines = []
    for name, _ in variants:
        st = stats(times[name])
        lines.append(json.dumps(dict({"what": "loss call", "variant": name, "B": B, "C": C, "reps": args.reps, "inner": args.inner}, **st,
                                     spread_ms=round(st["q75_ms"] - st["q25_ms"], 4), loss=round(float(out[name]), 5))))
    lines += [json.dumps(errors(ops, C)) for C in (64, 128, 256, 527, 1024, 1100)]
    for kernel, u in sorted(build.resource_usage().get("hinge.hip", {}).items()):
        lines.append(json.dumps({"what": "kernel resources", "kernel": kernel, "vgprs": u.get("VGPRs"), "sgprs": u.get("SGPRs"),
                                 "spilled_vgprs": u.get("VGPRs Spill"), "spilled_sgprs": u.get("SGPRs Spill"),
                                 "scratch_bytes_per_lane": u.get("ScratchSize [bytes/lane]"),
                                 "static_lds_bytes": u.get("LDS Size [bytes/block]"), "waves_per_simd": u.get("Occupancy [waves/SIMD]")}))
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
