"""Barlow Twins head alone (model/loss=barlow, reference layers [2048, 4096, 4096], E = 512): forward + backward of the HIP path
(ops.BarlowFn) against the same head composed from stock PyTorch ops under bf16 autocast, interleaved on one box, HIP events.

    python tools/barlow_bench.py [--batches 512 4096] [--iters 20] [--warmup 5]

Prints one JSON line per batch size: median ms of each path, their ratio, and the algorithmic TFLOP/s of the HIP path.  The stock
composition is here for comparison only; the product path never calls it."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def flops(B, sizes):
    proj = sum(2 * B * a * b for a, b in zip(sizes[:-1], sizes[1:]))         # one view's forward
    N = sizes[-1]
    return 2 * 3 * proj + 3 * 2 * B * N * N                                  # 2 views x (fwd + 2 bwd); c fwd + 2 bwd


def stock_loss(head, x1, x2):
    """The reference's forward (loss_head.py:313-328) from torch ops, bf16 autocast."""
    with torch.autocast("cuda", dtype=torch.bfloat16):
        z1, z2 = head.linear(x1), head.linear(x2)
        c = head.bn(z1).float().t() @ head.bn(z2).float()
    c = c / x1.shape[0]
    on = (torch.diagonal(c) - 1).pow(2).sum()
    off = c.pow(2).sum() - torch.diagonal(c).pow(2).sum()
    return on + head.lambd_off * off


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[512, 4096])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--hip-only", action="store_true", help="time the HIP path alone (for a kernel trace of just its launches)")
    args = ap.parse_args()
    import vipant_amd.module as M
    from vipant_amd import _ffi, ops
    from vipant_amd.config import to_config
    _ffi.call("vipant_device_check")
    layers = [2048, 4096, 4096]
    torch.manual_seed(0)
    head = M.build_loss_head(to_config({"name": "BarlowLossHead", "embed_dim": 512, "lambd_off": 0.0051,
                                        "layers": layers})).cuda().train()
    for B in args.batches:
        x1 = torch.randn(B, 512, device="cuda")
        x2 = (x1 + 0.5 * torch.randn(B, 512, device="cuda")).requires_grad_()

        def hip():
            head.zero_grad(set_to_none=True)
            head(x1, x2, normalized=False).backward(gradient=ops.unit_grad(x1.device))

        def stock():
            head.zero_grad(set_to_none=True)
            stock_loss(head, x1, x2).backward()

        times = {"hip": [], "stock": []}
        for it in range(args.warmup + args.iters):
            for name, fn in (("hip", hip),) + ((("stock", stock),) if not args.hip_only else ()):            # interleaved: both paths see the same clocks
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                if it >= args.warmup:
                    times[name].append(e0.elapsed_time(e1))
        med = {k: sorted(v)[len(v) // 2] if v else float("nan") for k, v in times.items()}
        print(json.dumps({"B": B, "layers": layers, "hip_ms": round(med["hip"], 4), "stock_bf16_autocast_ms": round(med["stock"], 4),
                          "hip_over_stock": round(med["hip"] / med["stock"], 3),
                          "hip_tflops": round(flops(B, [512] + layers) / med["hip"] / 1e9, 1),
                          "gflop": round(flops(B, [512] + layers) / 1e9, 1), "iters": args.iters}), flush=True)


if __name__ == "__main__":
    main()
