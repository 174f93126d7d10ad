"""Classification heads alone (model/loss=ce_cls, bce; E = 512): forward + backward of the HIP path (ops.ClassifierFn) against
the same head composed from stock PyTorch ops (fp32 LayerNorm, Linear under bf16 autocast, F.cross_entropy /
F.binary_cross_entropy_with_logits), interleaved on one box, HIP events.

    python tools/cls_bench.py [--shapes 50x50 512x50 512x527 4096x527] [--iters 30] [--warmup 5] [--hip-only]

Prints one JSON line per (B, C): median ms of each path and their ratio.  C = 527 runs the bce head (`bias: False`), the other
shapes the ce_cls head.  `--hip-only` times the HIP path alone, for a kernel trace of just its launches.  The stock composition
is here for comparison only; the product path never calls it."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def stock_loss(head, x, y):
    h = x
    mods = list(head.linear)
    for ln, lin in zip(mods[0::2], mods[1::2]):
        h = F.layer_norm(h.float(), (h.shape[1],), ln.weight, ln.bias, 1e-5)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            h = F.linear(h, lin.weight, lin.bias)
    logits = head.logit_scale.exp() * h.float()
    return F.cross_entropy(logits, y) if head.kind == "ce" else F.binary_cross_entropy_with_logits(logits, y.float())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["50x50", "512x50", "512x527", "4096x527"])
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--hip-only", action="store_true")
    args = ap.parse_args()
    import vipant_amd.module as M
    from vipant_amd import _ffi, ops
    from vipant_amd.config import to_config
    _ffi.call("vipant_device_check")
    torch.manual_seed(0)
    for shape in args.shapes:
        B, C = (int(v) for v in shape.split("x"))
        cfg = ({"name": "BCELossHead", "embed_dim": 512, "width": 768, "layers": [], "scaling": True, "bias": False} if C == 527
               else {"name": "ClassificationHead", "embed_dim": 512, "layers": [], "scaling": True})
        head = M.build_loss_head(to_config(cfg), output_dim=C).cuda().train()
        x = torch.randn(B, 512, device="cuda").requires_grad_()
        y = (torch.rand(B, C, device="cuda") < 0.01).to(torch.uint8) if C == 527 else torch.randint(0, C, (B,), device="cuda")

        def hip():
            head.zero_grad(set_to_none=True)
            head(x, y).backward(gradient=ops.unit_grad(x.device))

        def stock():
            head.zero_grad(set_to_none=True)
            stock_loss(head, x, y).backward()

        times = {"hip": [], "stock": []}
        for it in range(args.warmup + args.iters):
            for name, fn in (("hip", hip),) + ((("stock", stock),) if not args.hip_only else ()):      # interleaved: the same clocks
                with torch.no_grad():
                    head.linear[1].weight.add_(0.0)          # a new parameter version, as after an optimizer step: weights are re-cast
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                if it >= args.warmup:
                    times[name].append(e0.elapsed_time(e1))
        med = {k: sorted(v)[len(v) // 2] if v else float("nan") for k, v in times.items()}
        rec = {"B": B, "C": C, "head": cfg["name"], "hip_ms": round(med["hip"], 4)}
        if not args.hip_only:
            rec.update(stock_bf16_autocast_ms=round(med["stock"], 4), hip_over_stock=round(med["hip"] / med["stock"], 3))
        print(json.dumps(dict(rec, iters=args.iters)), flush=True)


if __name__ == "__main__":
    main()
