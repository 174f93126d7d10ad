"""VACELossHead's loss launch alone: the fused multi-pair call against the sequence it replaces -- one vipant_infonce_fwd_bwd call
per pair plus the fp32 adds that sum a shared operand's gradients -- interleaved in one process, warm, timed with device events:
    python tools/vace_bench.py [B] [reps]
Prints the median, minimum and maximum of both for the default graph of ce_va.yaml (vp, va, vv) and for all five pairs."""
import ctypes as C
import statistics
import sys

import torch

from vipant_amd import _ffi

DEV = "cuda:0"
GRAPHS = {"default (vp, va, vv)": (4, [(1, 0), (1, 2), (1, 3)]), "five pairs (vp, ap, va, vv, aa)": (5, [(1, 0), (2, 0), (1, 2), (1, 3), (2, 4)])}


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 432
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 40
    E = 512
    _ffi.call("vipant_device_check")
    stream = torch.cuda.current_stream().cuda_stream
    for name, (nop, pairs) in GRAPHS.items():
        npair = len(pairs)
        g = torch.Generator().manual_seed(B)
        base = torch.randn(B, E, generator=g)
        xs = []
        for _ in range(nop):
            x = base + 3.0 * torch.randn(B, E, generator=g)
            xs.append((x / x.norm(dim=-1, keepdim=True)).to(DEV))
        ls = torch.full((npair,), 2.6593, device=DEV)
        loss = torch.empty(npair + 1, device=DEV); dls = torch.empty(npair, device=DEV)
        dx = [None] + [torch.empty(B, E, device=DEV) for _ in range(nop - 1)]           # operand 0: the prime features, no gradient
        nb = _ffi.query("vipant_infonce_multi_workspace_bytes", B, E, nop, npair, B)
        ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
        xtab = (C.c_void_p * nop)(*[x.data_ptr() for x in xs])
        dtab = (C.c_void_p * nop)(*[None if d is None else d.data_ptr() for d in dx])
        pa, pb = (C.c_int32 * npair)(*[a for a, _ in pairs]), (C.c_int32 * npair)(*[b for _, b in pairs])
        zero, one = (C.c_float * npair)(), (C.c_float * npair)(*[1.0] * npair)

        def fused():
            _ffi.call("vipant_infonce_multi_fwd_bwd", xtab, nop, pa, pb, npair, ls.data_ptr(), zero, one, loss.data_ptr(), dtab,
                      dls.data_ptr(), 1.0, B, E, 0, B, ws.data_ptr(), nb, stream)

        nb1 = _ffi.query("vipant_infonce_strip_workspace_bytes", B, E, B)
        ws1 = torch.empty(nb1, dtype=torch.uint8, device=DEV)
        tmp = [(torch.empty(B, E, device=DEV), torch.empty(B, E, device=DEV)) for _ in pairs]
        l1, d1 = torch.empty(npair, device=DEV), torch.empty(npair, device=DEV)

        def sequence():
            acc = {}
            for k, (a, b) in enumerate(pairs):
                ta, tb = tmp[k]
                _ffi.call("vipant_infonce_fwd_bwd", xs[a].data_ptr(), xs[b].data_ptr(), ls[k:].data_ptr(), 0.0, l1[k:].data_ptr(),
                          ta.data_ptr(), None if dx[b] is None else tb.data_ptr(), d1[k:].data_ptr(), 1.0, B, E, 0, B, ws1.data_ptr(), nb1, stream)
                for i, t in ((a, ta), (b, tb)):
                    if dx[i] is None:
                        continue
                    if i in acc:
                        acc[i].add_(t)               # the fp32 add autograd makes for an operand shared by two terms
                    else:
                        acc[i] = t
            return acc

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3

        for _ in range(5):
            fused(); sequence()
        torch.cuda.synchronize()
        tf, ts = [], []
        for _ in range(reps):                       # interleaved: both see the same clocks and the same neighbours
            tf.append(timed(fused)); ts.append(timed(sequence))
        acc = sequence()
        fused()
        torch.cuda.synchronize()
        worst = max(float((acc[i] - dx[i]).abs().max() / acc[i].abs().max()) for i in acc)
        nadd = sum(sum(i in p for p in pairs) - 1 for i in range(1, nop))
        fmt = lambda t: f"median {statistics.median(t):7.1f} us  min {min(t):7.1f}  max {max(t):7.1f}  (quartiles {statistics.quantiles(t, n=4)[0]:.1f} / {statistics.quantiles(t, n=4)[2]:.1f})"
        print(f"B = {B}, E = {E}, {name}, {reps} interleaved repetitions, device events")
        print(f"  fused call (3 launches)                       {fmt(tf)}")
        print(f"  {npair} single-pair calls + {nadd} fp32 adds ({3 * npair + nadd} launches)   {fmt(ts)}")
        print(f"  per-pair losses equal bit for bit: {bool(torch.equal(loss[:npair], l1))}; largest gradient difference / scale: {worst:.2e}")


if __name__ == "__main__":
    main()
