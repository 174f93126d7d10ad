"""Cost of bringing a batch of clips to one sample rate on the device (`running.audio.resample_to`), HIP events.

    python tools/resample_bench.py [--reps 30] [--warmup 5] [--inner 4] [--out FILE]

One batch of b = 64 clips of 10 s of noise at 44100 Hz and at 48000 Hz, uploaded once, to 16000 Hz:
  launch  vipant_resample alone on prepared arguments, one output buffer (no host work);
  hip     frontend.Resample.__call__: the launch behind its wrapper (grouping by rate, the class array, fresh output tensors).
A repetition times `--inner` calls between two events and the variants take turns inside every repetition, so they see the same
clocks.  Per variant: median, quartiles, min / max of the per-call milliseconds; the bytes the rule needs (every input sample read
once, [b, out_stride] fp32 written once) over the median; the multiply-adds (T per output); and the time as a multiple of the traffic
floor -- those bytes over the 6.29 TB/s a float4 copy reaches on the part.  No threshold is asserted: the numbers are what was
observed."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tagging_bench import interleaved, stats  # noqa: E402

HBM_COPY_RATE = 6.29e12         # bytes/s of a float4 copy on the MI355X (8.0e12 is the specification)
B, SECONDS, TARGET = 64, 10.0, 16000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from vipant_amd import _ffi
    from vipant_amd.frontend import Resample
    _ffi.call("vipant_device_check")
    dev = torch.device("cuda:0")
    resample = Resample(TARGET, device=dev)
    variants, facts = [], {}
    for rate in (44100, 48000):
        n = int(SECONDS * rate)
        stride = -(-n // 8) * 8
        wave = torch.zeros((B, stride), dtype=torch.float32, device=dev)
        wave[:, :n] = torch.randn((B, n), generator=torch.Generator().manual_seed(rate)).to(dev)
        host = torch.full((B,), n, dtype=torch.int64)
        ns = host.to(dev)
        out, nout = resample(wave, ns, rate, host_lengths=host)
        plan = resample.plan(rate)
        assert nout.cpu().tolist() == resample.lengths(host, rate).tolist()
        classes, cls = (_ffi.ResampleClass * 1)(plan), (C.c_int32 * B)()
        argv = [wave.data_ptr(), stride, ns.data_ptr(), cls, classes, 1, out.data_ptr(), out.shape[1], nout.data_ptr(), B,
                torch.cuda.current_stream().cuda_stream]
        variants.append((f"launch_{rate}", lambda argv=argv, keep=(wave, ns, out, nout): _ffi.call("vipant_resample", *argv)))
        variants.append((f"hip_{rate}", lambda wave=wave, ns=ns, rate=rate, host=host: resample(wave, ns, rate, host_lengths=host)))
        for name in (f"launch_{rate}", f"hip_{rate}"):
            facts[name] = {"rate": rate, "samples": n, "out_stride": out.shape[1], "T": plan.T, "P": plan.P, "lds_bytes": plan.lds_bytes,
                           "needed_bytes": B * (n + out.shape[1]) * 4, "fma": B * int(nout[0]) * plan.T}
    times = interleaved(tuple(variants), args.reps, args.warmup, args.inner)
    lines = []
    for name, fn in variants:
        t0 = time.perf_counter()
        for _ in range(20):
            fn()
        host_ms = (time.perf_counter() - t0) / 20 * 1e3      # enqueue only: nothing here waits for the stream
        torch.cuda.synchronize()
        st, f = stats(times[name]), facts[name]
        floor_ms = f["needed_bytes"] / HBM_COPY_RATE * 1e3
        lines.append(json.dumps(dict({"what": "resample", "variant": name, "b": B, "target": TARGET, "reps": args.reps, "inner": args.inner},
                                     **f, **st, spread_ms=round(st["q75_ms"] - st["q25_ms"], 4),
                                     needed_TB_per_s=round(f["needed_bytes"] / (st["median_ms"] * 1e-3) / 1e12, 3),
                                     TFMA_per_s=round(f["fma"] / (st["median_ms"] * 1e-3) / 1e12, 3), floor_ms=round(floor_ms, 4),
                                     fraction_of_floor_rate=round(floor_ms / st["median_ms"], 3), host_enqueue_ms=round(host_ms, 4))))
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
