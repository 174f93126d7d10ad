"""Cost of the LAMB step beside the fused Adam step, interleaved on one box, HIP events.

    python tools/lamb_bench.py [--reps 30] [--warmup 5] [--inner 4] [--out profiles/lamb_observed.txt]

One step over the trainable parameter list of the headline VA model (tools/adam_bench.py: headline_shapes), random parameters and
gradients, every variant on its own copy of the same values:
  adam            vipant_amd.module.Adam: one vipant_adam_step launch, 28 B per element;
  lamb_clip       vipant_amd.module.LAMB(max_grad_norm=1): five launches, 44 B per element;
  lamb            vipant_amd.module.LAMB(max_grad_norm=0): three launches, 40 B per element;
  lamb_plain      LAMB(max_grad_norm=1, fused=False): the class's plain torch step;
  launch_*        vipant_adam_step / vipant_lamb_step alone on prepared tables (no host work), clip on / off, 4- and 16-byte accesses;
  grad_norm       ops.grad_norm over the gradients (tables built per call).
A repetition times `--inner` steps between two events and the variants take turns inside every repetition, so they see the same
clocks.  Per variant: median, quartiles, min / max of the per-step milliseconds, the spread q75 - q25, the bytes the rule needs over the
median, and the host's time to enqueue a step; one JSON line each.  Before anything is timed the fused and the plain LAMB step are
compared after one step, and the kernels' register counts are reported from the build."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from adam_bench import headline_shapes  # noqa: E402
from tagging_bench import interleaved, stats  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import vipant_amd.module as M
    from vipant_amd import _ffi, build, ops
    _ffi.call("vipant_device_check")
    dev = torch.device("cuda:0")
    shapes = headline_shapes(dev)
    torch.cuda.empty_cache()
    nelem = sum(int(torch.Size(s).numel()) for s in shapes)

    def make(cls, **kw):
        g = torch.Generator(device=dev).manual_seed(11)
        params = [torch.nn.Parameter(torch.randn(s, generator=g, device=dev)) for s in shapes]
        for p in params:
            p.grad = torch.randn(p.shape, generator=g, device=dev) * 1e-2
        return params, cls([{"params": [p for p in params if p.ndim > 1]}, {"params": [p for p in params if p.ndim < 2]}], lr=1e-3, **kw)

    built = {"adam": make(M.Adam, weight_decay=1e-6), "lamb_clip": make(M.LAMB, max_grad_norm=1.0), "lamb": make(M.LAMB, max_grad_norm=0.0),
             "lamb_plain": make(M.LAMB, max_grad_norm=1.0, fused=False)}
    bytes_per_element = {"adam": 28, "lamb_clip": 44, "lamb": 40, "lamb_plain": 44, "grad_norm": 4}
    for _, opt in built.values():
        opt.step()
    torch.cuda.synchronize()
    diff = max(float((p.detach() - q.detach()).abs().max()) for p, q in zip(built["lamb_clip"][0], built["lamb_plain"][0]))
    assert diff <= 1e-5, diff                             # parameters ~ N(0, 1), the largest of 88 M near 6: a few ulps of that
    state = built["lamb_clip"][1]._vipant_fused[1]
    stream = torch.cuda.current_stream().cuda_stream
    grads = [p.grad for p in built["lamb_clip"][0]]

    def with_width(env, width, fn):
        def run():
            os.environ[env] = str(width)
            try:
                fn()
            finally:
                del os.environ[env]
        return run

    adam_state = built["adam"][1]._vipant_fused
    adam_state = next(iter(adam_state.values()))[1]
    adam_argv = (adam_state.p_ptrs.data_ptr(), adam_state.g_ptrs.data_ptr(), adam_state.m_ptrs.data_ptr(), adam_state.v_ptrs.data_ptr(),
                 adam_state.n.data_ptr(), adam_state.rec.data_ptr(), adam_state.chunk_start.data_ptr(), len(shapes), adam_state.nchunks,
                 adam_state.chunk, 0.9, 0.999, 0, stream)
    lamb_argv = (state.p_ptrs.data_ptr(), state.g_ptrs.data_ptr(), state.m_ptrs.data_ptr(), state.v_ptrs.data_ptr(), state.n.data_ptr(),
                 state.rec.data_ptr(), state.chunk_start.data_ptr(), len(shapes), state.nchunks, state.chunk, 0.9, 0.999)
    ws = (state.ws.data_ptr(), state.ws.numel(), stream)
    kernels = []
    for w in (4, 16):
        kernels.append((f"launch_adam_w{w}", with_width("VIPANT_ADAM_WIDTH", w, lambda: _ffi.call("vipant_adam_step", *adam_argv))))
        bytes_per_element[f"launch_adam_w{w}"] = 28
        for name, mgn, nbytes in (("clip", 1.0, 44), ("noclip", 0.0, 40)):
            kernels.append((f"launch_lamb_{name}_w{w}", with_width("VIPANT_LAMB_WIDTH", w, lambda mgn=mgn: _ffi.call("vipant_lamb_step", *lamb_argv, mgn, *ws))))
            bytes_per_element[f"launch_lamb_{name}_w{w}"] = nbytes
    variants = tuple((name, opt.step) for name, (_, opt) in built.items()) + tuple(kernels) + (("grad_norm", lambda: ops.grad_norm(grads)),)
    usage = {k.split("N_1", 1)[-1]: {f: u[f] for f in ("VGPRs", "VGPRs Spill", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]")}
             for k, u in build.resource_usage().get("lamb.hip", {}).items()}
    lines = [json.dumps({"what": "lamb step check", "tensors": len(shapes), "elements": nelem, "chunks": state.nchunks,
                         "max_abs_diff_fused_vs_plain_after_one_step": diff, "G": float(state.grad_norm), "c": float(state.clip_coef)}),
             json.dumps({"what": "lamb.hip resource usage", "kernels": usage})]
    times = interleaved(variants, args.reps, args.warmup, args.inner)
    for name, fn in variants:
        t0 = time.perf_counter()
        for _ in range(20):
            fn()
        host = (time.perf_counter() - t0) / 20 * 1e3      # enqueue only: nothing here waits for the stream
        torch.cuda.synchronize()
        st = stats(times[name])
        lines.append(json.dumps(dict({"what": "lamb step", "variant": name, "reps": args.reps, "inner": args.inner}, **st,
                                     spread_ms=round(st["q75_ms"] - st["q25_ms"], 4),
                                     rule_TB_per_s=round(bytes_per_element[name] * nelem / (st["median_ms"] * 1e-3) / 1e12, 3),
                                     host_enqueue_ms=round(host, 4))))
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
