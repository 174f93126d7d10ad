"""LayerNorm at the widths that are no multiple of 256 against the yardstick a user has today: padding to the next multiple of 256.

For each pair (D, next multiple of 256 above D) the forward and the backward launch of a transformer block as the headline step issues
them (fp16 stream in and out, bf16 residual branch added in front of the norm, bf16 output; backward with bf16 dy, fp16 rows, bf16
residual gradient, bf16 dx) are timed at equal M in one process, in alternating rounds, with HIP events.  Reported: median and
interquartile spread in us, GB/s over the bytes the launch has to move (8 B per element each way), and whether the new width is no
slower than the padded one within the larger of the two spreads.

    python tools/ln_widths_bench.py [--rows 161792] [--rounds 40] [--pairs 192:256,384:512,640:768,960:1024] [--label TEXT] [--out FILE]

VIPANT_HIP_LIB selects another build of the library (a forced group size: -DVIPANT_LN_LANES=16|32|64 on layernorm_widths.hip)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from vipant_amd import _ffi  # noqa: E402

DEV = "cuda:0"


def make(M, D):
    g = torch.Generator(device=DEV).manual_seed(D)
    r = lambda *s, dt: torch.randn(*s, generator=g, device=DEV).to(dt)
    t = dict(x=r(M, D, dt=torch.float16), add=r(M, D, dt=torch.bfloat16), gamma=r(D, dt=torch.float32), beta=r(D, dt=torch.float32),
             y=torch.empty(M, D, dtype=torch.bfloat16, device=DEV), xs=torch.empty(M, D, dtype=torch.float16, device=DEV),
             mean=torch.empty(M, device=DEV), rstd=torch.empty(M, device=DEV), dy=r(M, D, dt=torch.bfloat16), dres=r(M, D, dt=torch.bfloat16),
             dg=torch.empty(D, device=DEV), db=torch.empty(D, device=DEV))
    t["ws"] = torch.empty(_ffi.query("vipant_layernorm_bwd_workspace_bytes", M, D), dtype=torch.uint8, device=DEV)
    return t


def fwd(t, M, D, s):
    _ffi.call("vipant_layernorm_fwd", t["x"].data_ptr(), D, t["gamma"].data_ptr(), t["beta"].data_ptr(), t["y"].data_ptr(), None,
              t["mean"].data_ptr(), t["rstd"].data_ptr(), M, D, t["add"].data_ptr(), t["xs"].data_ptr(), None, None,
              _ffi.STREAM_IN_F16 | _ffi.STREAM_OUT_F16, s)


def bwd(t, M, D, s):            # the residual gradient is updated in place, as in the stack (dres == dx_bf16)
    _ffi.call("vipant_layernorm_bwd", t["dy"].data_ptr(), _ffi.LN_DRES_BF16 | _ffi.LN_X_F16, t["xs"].data_ptr(), D, t["mean"].data_ptr(),
              t["rstd"].data_ptr(), t["gamma"].data_ptr(), t["dres"].data_ptr(), None, D, t["dres"].data_ptr(), t["dg"].data_ptr(),
              t["db"].data_ptr(), None, 0, M, D, t["ws"].data_ptr(), t["ws"].numel(), None, None, s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=161792)
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--pairs", default="192:256,384:512,640:768,960:1024")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ln_widths_bench: no GPU (timings come from the device only)")
    M, s = a.rows, torch.cuda.current_stream().cuda_stream
    lines = [f"# {a.label or 'library: ' + _ffi.LIB_PATH}; M = {M}, {a.rounds} alternating rounds; us = median (interquartile spread)"]
    for pair in a.pairs.split(","):
        Dn, Do = (int(v) for v in pair.split(":"))
        data = {D: make(M, D) for D in (Dn, Do)}
        for name, fn in (("fwd", fwd), ("bwd", bwd)):
            times = {Dn: [], Do: []}
            for rnd in range(a.rounds + 5):          # five warm-up rounds
                for D in (Dn, Do):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(); fn(data[D], M, D, s); e1.record()
                    e1.synchronize()
                    if rnd >= 5:
                        times[D].append(e0.elapsed_time(e1) * 1e3)
            med = {D: statistics.median(v) for D, v in times.items()}
            q = {D: statistics.quantiles(v, n=4) for D, v in times.items()}
            iqr = {D: q[D][2] - q[D][0] for D in q}
            ok = med[Dn] <= med[Do] + max(iqr.values())
            lines.append(f"{name} D={Dn:4d} {med[Dn]:7.1f} ({iqr[Dn]:4.1f}) us {8 * M * Dn / med[Dn] / 1e3:6.0f} GB/s | D={Do:4d} {med[Do]:7.1f} "
                         f"({iqr[Do]:4.1f}) us {8 * M * Do / med[Do] / 1e3:6.0f} GB/s | {'no slower' if ok else 'SLOWER'} than padding")
        del data
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
