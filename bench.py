"""Benchmark of the hot path: one full VA pre-training step of VIP-ANT's bimodal contrastive objective on synthetic
data -- frozen CLIP ViT-B/32 image tower (forward) + trainable audio ViT-B (forward + backward) + InfoNCE over the
global batch + gradient all-reduce + LARS step.  Workload = BASELINE.json configs[1] per GPU (batch 512,
128-bin x 1024-frame spectrograms, S = 316 tokens); with N GPUs the global batch is 512 * N (configs[3] at N = 8).

    python bench.py --gpus 1 --steps 5 --warmup 2
    python bench.py --gpus 1 --steps 5 --warmup 2 --full          # + the extra measurements listed below
    python bench.py --gpus 1 --steps 5 --warmup 2 --dump-outputs DIR
    python bench.py --gpus N --steps K --warmup W        # starts its own N replicas (child torch.distributed.run, RCCL)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W           # the driver's form: already under a launcher, runs as one replica

Prints ONE JSON line on rank 0: metric / value / unit / ms_per_step of the timed steps.  A plain run does nothing else: set-up,
warm-up, the timed steps, the outputs (--dump-outputs), the line.  With --full the line also carries the roofline of the dominant
kernel (c_fc forward contraction, timed with HIP events in the timed steps and in a serial post-pass), the InfoNCE group and the
audio encoder alone, the step with the full last block, and cpu_baseline (the CPU oracle on the host cores); the --no-* options
switch single ones of these off.

--dump-outputs DIR writes what the last timed step computed, as float32 / float64 .npy files (at most 48 MiB; 18 MB at the headline):
loss.npy (the loss the step returned), params.npy and grads.npy (a fixed, seeded sample of every trainable parameter after the
optimizer step and of its gradient, the same elements in both, parameters in name order).  The inputs, the initial weights and
the sample are seeded: the same arguments give the same inputs on every run.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# torch (and with it the HIP runtime) is imported by main(), AFTER the decision whether this process is a replica or the parent that
# starts the replicas: the parent of `python bench.py --gpus N` must never touch the GPU (vipant_amd/launch.py)
torch = dist = None

PEAK_BF16_TFLOPS = 2500.0          # dense MFMA peak, /opt/skills/guides/MI355X_MICROARCH.md
D, L, E, HEADS = 768, 12, 512, 12
DOMINANT_KERNEL = "gemm_nt_pp_kernel<6, 12, 2, 0, true>"      # c_fc forward + QuickGELU, 8-bit QuickGELU' code (name as rocprofv3 prints it)


def tower_fwd_flops(S, kpatch, P, width=D, layers=L, embed=E, last_block_rows=False):
    """L*S*(24 D^2 + 4 S D) + 2 P Kpatch D + 2 D E per sample.  With `running.last_block_rows` the last block
    is evaluated on the one row per item the read-out takes, and what is counted is the work the step then actually needs:
    round-3 form (`VIPANT_LAST_BLOCK_CTX=0`, or a width / length the folded kernels do not take): the key / value projection of
    every token (4 S D^2) + everything else on one row (20 D^2 + 4 S D); default (key / value projection folded into the query
    side, csrc/readout_ctx.hip): one row's 24 D^2 (the two folded projections are D x D per item) + scores and contexts against
    the LayerNorm output, 4 S H D with H = D / 64.  The zeros of the block-sparse head expansion are not counted."""
    full = S * (24 * width * width + 4 * S * width)
    folded = os.environ.get("VIPANT_LAST_BLOCK_CTX", "1") != "0" and width in (512, 768, 1024) and S <= 1024
    if not (last_block_rows and layers > 0):
        last = full
    elif folded:
        last = 24 * width * width + 4 * S * (width // 64) * width
    else:
        last = 4 * S * width * width + 20 * width * width + 4 * S * width
    return (layers - 1) * full + last + 2 * P * kpatch * width + 2 * width * embed if layers > 0 else 2 * P * kpatch * width + 2 * width * embed


PMC_FILE = "profiles/r6_pmc_traffic.json"      # this round's counter passes on the shipped build (tools/round_batch.sh pmc)


def pmc_traffic(M, N, K):
    """HBM bytes per launch of the dominant kernel from the committed rocprofv3 PMC passes (PMC_FILE: FETCH_SIZE x 2 +
    WRITE_SIZE, separate --pmc passes; that file holds the commands, the build it was taken on and the kernel name).  The
    counters cannot be collected inside this process, so the bench line names the file the number came from (`traffic_source`)
    and reports None when the file has no entry for the kernel / shape that is being timed."""
    try:
        with open(os.path.join(ROOT, PMC_FILE)) as f:
            k = json.load(f)["kernels"].get(f"{DOMINANT_KERNEL} M={M} N={N} K={K}")
        return None if k is None else k["fetch_bytes"] + k["write_bytes"]
    except (OSError, KeyError, ValueError):
        return None


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=512, help="per-GPU batch (configs[1]: 512)")
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--mels", type=int, default=128)
    ap.add_argument("--layers", type=int, default=L)
    ap.add_argument("--width", type=int, default=D, help="audio tower width (heads = width // 64, cvap/module/val.py:474); "
                    "1024 with --layers 24 is the audio ViT-L of BASELINE configs[4]")
    ap.add_argument("--recompute-mlp", action="store_true", help="running.recompute_mlp: MLP activations re-made in the backward")
    ap.add_argument("--fp8", action="store_true", help="running.fp8_gemm: e4m3 operands in the audio tower's NT contractions "
                                                       "(BASELINE.json configs[4]; never the headline line, which is bf16)")
    ap.add_argument("--micro-batch", type=int, default=0, help="running.micro_batch: towers in micro-batches under one loss")
    ap.add_argument("--stream", choices=["fp32", "fp16"], default=None,
                    help="running.stream_dtype: precision of the residual stream inside the transformer stacks (default: the "
                         "framework's default)")
    ap.add_argument("--full-last-block", action="store_true",
                    help="running.last_block_rows=False: evaluate the towers' last block on every token, as the reference does before "
                         "its read-out discards all rows but one (default: on the read-out rows only -- exact up to rounding order, see DESIGN.md)")
    ap.add_argument("--no-full-last-block-check", action="store_true",
                    help="--full: skip the 8 extra steps that report the step time with the full last block beside the headline")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU oracle's timing")
    ap.add_argument("--no-encoder-alone", action="store_true", help="--full: skip the 13 extra audio-encoder-only iterations (profiling runs: the "
                    "per-step kernel tables divide by the number of whole steps)")
    ap.add_argument("--script", choices=["va", "at"], default="va",
                    help="va: BASELINE configs[1]/[3] (the headline; frozen image tower).  at: configs[2] -- audio tower + frozen "
                         "CLIP text tower at L=77, local negatives (run_bimodal_at.sh); extra measurement, not the headline")
    ap.add_argument("--cpu-batch", type=int, default=64)
    ap.add_argument("--full", action="store_true",
                    help="also the extra measurements (roofline of the dominant kernel, InfoNCE and audio encoder alone, full last "
                         "block, CPU baseline); a plain run times the steps and nothing else")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's loss and a seeded sample of the updated parameters and their gradients to DIR/*.npy")
    ap.add_argument("--comm-overlap", choices=["block", "step"], default="block",
                    help="running.comm_overlap: replicas reduce each block's gradient bucket while the blocks below run their backward "
                         "(block, default) or all buckets as one collective after the backward (step)")
    return ap.parse_args()


def host_cpu():
    """(model name, usable cores) of this box: lscpu's sockets x cores per socket, capped by the process's CPU affinity and by
    the cgroup CPU quota."""
    import subprocess
    model, cores_per_socket, sockets = "unknown", None, None
    try:
        for line in subprocess.run(["lscpu"], capture_output=True, text=True, timeout=10).stdout.splitlines():
            key, _, val = line.partition(":")
            key, val = key.strip(), val.strip()
            if key == "Model name":
                model = val
            elif key == "Core(s) per socket":
                cores_per_socket = int(val)
            elif key == "Socket(s)":
                sockets = int(val)
    except Exception:
        pass
    physical = cores_per_socket * sockets if cores_per_socket and sockets else (os.cpu_count() or 1)
    # the cores this process may actually use: CPU affinity and the cgroup CPU quota of the box (more threads than that are
    # throttled: a 16-CPU quota under 128 threads ran the same sample 3-5x slower, and differently from run to run)
    try:
        physical = max(1, min(physical, len(os.sched_getaffinity(0))))
    except (AttributeError, OSError):
        pass
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            physical = max(1, min(physical, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return model, physical


def cpu_baseline(args, T, Fq):
    """The CPU oracle (oracle/ref_cpu.py, pinned against the reference by tests/golden) timed on this box's host cores,
    SURVEY.md 8-D5 protocol, `torch.set_num_threads(physical cores)`:
      * cfg1 exactly (BASELINE.json configs[0]): batch 32, 256 x 64 spectrograms, precomputed image embeddings, fp32,
        forward + backward + LARS, 2 warm-up + 5 timed steps, median;
      * the headline workload's shapes (configs[1]) on a bounded sample: `--cpu-batch` pairs, image tower forward + audio
        tower forward / backward + InfoNCE + LARS, 1 warm-up (2 pairs) + 1 timed step -- `value` is this leg's pairs/s."""
    from oracle import ref_cpu as R
    model, physical = host_cpu()
    torch.set_num_threads(physical)
    torch.manual_seed(0)

    def rand_sd(shapes, grad):
        sd = {}
        for k, shp in shapes.items():
            if k.endswith("ln.weight") or k.endswith("ln_1.weight") or k.endswith("ln_2.weight"):
                t = torch.ones(shp)
            elif k.endswith("bias"):
                t = torch.zeros(shp)
            else:
                t = torch.randn(shp) * (shp[-1] ** -0.5 if len(shp) > 1 else 0.02)
            sd[k] = t.requires_grad_(grad)
        return sd

    def lars_all(params, mus, lw, lb):
        with torch.no_grad():
            for k, v in params.items():
                if v.grad is None:
                    continue
                p_new, mus[k] = R.lars_step(v.detach(), v.grad, mus[k], lw if v.ndim > 1 else lb)
                v.copy_(p_new)
                v.grad = None

    # ---- leg 1: cfg1 exactly
    b1, T1, F1 = 32, 256, 64
    stride1, S1, pr1 = R.vit_position_resolution([T1, F1], 32, [16, 24])
    sd1 = rand_sd(R.audio_head_shapes(D, L, E, S1), True)
    ls1 = torch.tensor(2.6593, requires_grad=True)
    p1 = dict(sd1, logit_scale=ls1)
    mu1 = {k: torch.zeros_like(v) for k, v in p1.items()}
    aud1, img1 = torch.randn(b1, 1, T1, F1), torch.randn(b1, E)
    times = []
    for it in range(7):
        t0 = time.perf_counter()
        lw, lb = R.adjust_learning_rate(it + 10, epochs=1000, steps_per_epoch=10, warmup_epoch=10, batch_size=b1,
                                        lr_weight=0.2, lr_bias=0.0048)
        fa = R.vit_head_forward(aud1, sd1, width=D, layers=L, stride=stride1, position_resolution=pr1)
        loss = R.ce_loss_head(R.l2_normalize(img1), fa, ls1)
        loss.backward()
        lars_all(p1, mu1, lw, lb)
        times.append(time.perf_counter() - t0)
    t_cfg1 = sorted(times[2:])[2]

    # ---- leg 2: bounded sample at the headline shapes
    b = args.cpu_batch
    stride, S, pr = R.vit_position_resolution([T, Fq], 32, [16, 24])
    asd = rand_sd(R.audio_head_shapes(D, args.layers, E, S), True)
    isd = rand_sd(R.audio_head_shapes(D, args.layers, E, 50), False)
    ls = torch.tensor(2.6593, requires_grad=True)
    p2 = dict(asd, logit_scale=ls)
    mu2 = {k: torch.zeros_like(v) for k, v in p2.items()}

    def step(n):
        aud, img = torch.randn(n, 1, T, Fq), torch.randn(n, 3, 224, 224)
        with torch.no_grad():
            fi = R.vit_head_forward(img, isd, width=D, layers=args.layers, stride=[32, 32], position_resolution=(7, 7))
        fa = R.vit_head_forward(aud, asd, width=D, layers=args.layers, stride=stride, position_resolution=pr)
        R.ce_loss_head(fi, fa, ls).backward()
        lars_all(p2, mu2, 0.4, 0.0096)
    step(2)
    t0 = time.perf_counter()
    step(b)
    dt = time.perf_counter() - t0
    return {"value": round(b / dt, 3), "unit": "pairs/s", "cores": physical, "kind": "port", "cpu_model": model,
            "threads": torch.get_num_threads(),
            "sample": f"1 timed step of {b} pairs at the headline shapes ({T}x{Fq} spectrograms, 3x224x224 images, {args.layers} "
                      f"layers), fp32 oracle incl. LARS, after a 2-pair warm-up; {dt:.1f} s",
            "cfg1": {"workload": "BASELINE.json configs[0]: batch 32, 256x64 spectrograms, precomputed image embeddings, fp32, "
                                 "fwd + bwd + LARS; 2 warm-up + 5 timed steps, median",
                     "median_step_s": round(t_cfg1, 3), "pairs_per_s": round(b1 / t_cfg1, 2)}}


DUMP_ELEMENTS = 6 << 20        # elements per sampled array of --dump-outputs (float32): params.npy + grads.npy <= 48 MiB


def dump_outputs(path, model, loss):
    """What the last timed step gave its caller, as <path>/<name>.npy: the loss it returned (float64), the trainable parameters
    after its optimizer step and the gradients it left on them (float32).  Parameters and gradients are a fixed sample of the same
    elements: parameters in name order, each one whole when it is smaller than an equal share of DUMP_ELEMENTS, else that share at
    seeded positions (sorted)."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    named = [(k, p) for k, p in model.named_parameters() if p.requires_grad]
    share = DUMP_ELEMENTS // max(len(named), 1)
    gen = torch.Generator().manual_seed(0)
    vals, grads = [], []
    for _, p in named:
        flat = p.detach().reshape(-1)
        n = flat.numel()
        idx = torch.arange(n) if n <= share else torch.randint(0, n, (share,), generator=gen).sort().values
        idx = idx.to(flat.device)
        vals.append(flat[idx].float())
        grads.append(p.grad.detach().reshape(-1)[idx].float() if p.grad is not None else torch.zeros(idx.numel(), device=flat.device))
    np.save(os.path.join(path, "loss.npy"), np.array([float(loss.detach())], dtype=np.float64))
    np.save(os.path.join(path, "params.npy"), torch.cat(vals).cpu().numpy())
    np.save(os.path.join(path, "grads.npy"), torch.cat(grads).cpu().numpy())


def bench_at(args, world, rank, local_rank, dev, use_dist):
    """AT fine-tuning step (BASELINE configs[2]): trainable audio head, frozen causal text tower, VALCELossHead(al)."""
    from vipant_amd import _ffi
    from vipant_amd.config import compose
    from vipant_amd.monitor import VALMonitor
    from vipant_amd.module import adjust_learning_rate
    _ffi.call("vipant_device_check")
    T, Fq, b = args.frames, args.mels, args.batch
    ov = ("+running=trimodal monitor=VALMonitor worker=CVALP mode=ddp eval=False +model/image=vit_val +model/audio=vit_val "
          "+model/text=transformer_val +model/loss=ce_val +optimizer=standard +running/audio=default "
          "model.audio.pre_encoder.in_channels=3 model.audio.pre_encoder.stride=[16,24] running.siamese.alive=True "
          f"running.imagine=False model.loss.va=False model.image.encoder.layers={min(args.layers, 12)} "
          f"model.audio.width={args.width} model.audio.encoder.layers={args.layers} +running.negatives=local "
          f"running.recompute_mlp={args.recompute_mlp} running.micro_batch={args.micro_batch} running.fp8_gemm={args.fp8} "
          + (f"running.stream_dtype={args.stream} " if args.stream else "") + f"running.last_block_rows={not args.full_last_block} " +
          f"running.audio.max_len={T} running.audio.num_mel_bins={Fq} running.batch_size={b} running.epochs=1000 "
          f"running.save_epoch=False running.save_rate=1e9 running.peep_rate=1000000 "
          f"running.synthetic_steps={args.steps + args.warmup} num_gpus={world}").split()
    cfg = compose(ov)
    cfg.rank = rank
    torch.manual_seed(cfg.seed)
    mon = VALMonitor(cfg, (lambda *_: None), dev)
    mon.total_loss = mon.total_step = mon.total_inst = 0
    mon.start_time = time.time()
    images, audios, text, _, _ = mon.make_batch(next(iter(mon.dataloader)))
    text = torch.cat([text, text.new_zeros(text.shape[0], 77 - text.shape[1])], dim=1) if text.shape[1] < 77 else text

    def one_step(i):
        adjust_learning_rate(cfg.optimizer, mon.optimizer, mon.dataloader, i + 10)
        return mon.step(images, audios, text)

    for i in range(args.warmup):
        one_step(i)
    if use_dist:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        loss = one_step(args.warmup + i)
    if use_dist:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if use_dist:
        tmax = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = float(tmax)
    ms = dt / args.steps * 1e3
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, mon.model, loss)
    S = mon.model.audio_head.misc.positional_embedding.shape[0]
    # algorithmic work of the step (recomputation and the micro-batch pre-pass are NOT counted as work done)
    lbr = not args.full_last_block
    algo_flops = b * (3 * tower_fwd_flops(S, 1024, S - 1, width=args.width, layers=args.layers, last_block_rows=lbr)
                      + tower_fwd_flops(77, 0, 0, width=512, layers=12, last_block_rows=lbr)) + 6.0 * b * b * E
    out = {"metric": "audio_text_pairs_per_sec", "value": round(b * world / (ms * 1e-3), 2), "unit": "pairs/s", "n_gpus": world,
           "ranks": world, "rccl": dist.get_backend() if use_dist else None, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms, 3), "higher_is_better": True, "scaling": "weak",
           "vs_baseline": None, "dtype": ("e4m3 contractions (NT and weight-gradient), bf16 elsewhere" if os.environ.get("VIPANT_FP8_TN", "1") != "0" else "e4m3 NT contractions, bf16 elsewhere") if args.fp8 else "bf16", "data": "synthetic",
           "config": {"workload": f"AT fine-tuning step, per-GPU batch {b}, {Fq}-bin x {T}-frame spectrograms (S={S}), audio ViT width "
                                  f"{args.width} / {args.layers}L fwd+bwd + frozen CLIP text tower (L=77) fwd + InfoNCE(al) + LARS, local "
                                  "negatives (BASELINE.json configs[2]; configs[4]'s tower with --width 1024 --layers 24, bf16 weights); "
                                  "NOT the headline configuration",
                      "global_batch": b * world, "tokens_per_sample": int(S), "parallelism": f"dp{world}", "negatives": "local",
                      "recompute_mlp": bool(args.recompute_mlp), "micro_batch": int(args.micro_batch), "fp8_gemm": bool(args.fp8),
                      "last_block": "read-out rows only (exact up to bf16 rounding order)" if lbr else "every token"},
           "loss": round(float(loss.detach()), 4), "step_tflops": round(algo_flops / (ms * 1e-3) / 1e12, 1),
           "step_mfma_frac": round(algo_flops / (ms * 1e-3) / 1e12 / PEAK_BF16_TFLOPS, 4),
           "peak_mem_gb": round(torch.cuda.max_memory_allocated() / 1e9, 1)}
    if rank == 0:
        print(json.dumps(out), flush=True)
    if use_dist:
        dist.destroy_process_group()


def main():
    args = parse()
    from vipant_amd import launch
    if args.gpus > 1 and not launch.under_launcher():
        # `python bench.py --gpus N`: N replicas as a child process, started before anything here has touched the GPU
        sys.exit(launch.replicas(os.path.abspath(__file__), sys.argv[1:], args.gpus))
    global torch, dist
    import torch
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        sys.stderr.write(f"[bench] --gpus {args.gpus} but the launcher started {world} replica(s): reporting n_gpus = {world}\n")
    rank = int(os.environ.get("RANK", "0"))
    # one rank per GPU; with fewer visible GPUs than ranks (the 2-rank test on a 1-GPU box) ranks share devices round-robin
    local_rank, ndev = int(os.environ.get("LOCAL_RANK", "0")), max(torch.cuda.device_count(), 1)
    if os.environ.get("VIPANT_DIST_BACKEND", "nccl") == "nccl" and local_rank >= ndev:
        raise RuntimeError(f"LOCAL_RANK {local_rank} but only {ndev} visible GPU(s): RCCL takes one GPU per rank")
    local_rank %= ndev
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    use_dist = world > 1 or ("RANK" in os.environ and "MASTER_ADDR" in os.environ)      # launched by torch.distributed.run
    if use_dist:
        backend = os.environ.get("VIPANT_DIST_BACKEND", "nccl")        # "nccl" = RCCL over xGMI; "gloo" only for the shared-GPU test
        if backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=dev)
        else:
            dist.init_process_group(backend=backend)

    from vipant_amd import _ffi, ops
    from vipant_amd.config import compose
    from vipant_amd.monitor import VAMonitor
    from vipant_amd.module import adjust_learning_rate
    _ffi.call("vipant_device_check")

    T, Fq, b = args.frames, args.mels, args.batch
    if args.script == "at":
        return bench_at(args, world, rank, local_rank, dev, use_dist)
    ov = ("+running=bimodal worker=CVALP mode=ddp eval=False +model/image=vit_val +model/audio=vit_val +model/text=dummy "
          "+model/loss=ce +optimizer=standard +running/audio=default model.audio.pre_encoder.in_channels=3 "
          f"model.audio.pre_encoder.stride=[16,24] model.image.encoder.layers={min(args.layers, 12)} "
          f"model.audio.width={args.width} model.audio.encoder.layers={args.layers} "
          f"running.recompute_mlp={args.recompute_mlp} running.micro_batch={args.micro_batch} running.fp8_gemm={args.fp8} "
          + (f"running.stream_dtype={args.stream} " if args.stream else "") + f"running.last_block_rows={not args.full_last_block} " +
          f"running.audio.max_len={T} running.audio.num_mel_bins={Fq} running.comm_overlap={args.comm_overlap} "
          f"running.batch_size={b} running.epochs=1000 running.save_epoch=False running.save_rate=1e9 running.peep_rate=1000000 "
          f"running.synthetic_steps={args.steps + args.warmup} num_gpus={world}").split()
    cfg = compose(ov)
    cfg.rank = rank
    torch.manual_seed(cfg.seed)
    mon = VAMonitor(cfg, (lambda *_: None), dev)
    mon.total_loss = mon.total_step = mon.total_inst = 0
    mon.start_time = time.time()

    # synthetic batch already resident in HBM (the timed region excludes H2D, as the contract requires)
    g = torch.Generator().manual_seed(1213 + rank)
    images = torch.randn(b, 3, 224, 224, generator=g).to(dev)
    audios = torch.randn(b, 1, T, Fq, generator=g).to(dev)

    def one_step(i):
        adjust_learning_rate(cfg.optimizer, mon.optimizer, mon.dataloader, i + 10)
        return mon.step(images, audios, None)

    for i in range(args.warmup):
        one_step(i)
    S = mon.model.audio_head.misc.positional_embedding.shape[0]
    Mrows = b * S
    W = args.width
    if args.full:
        # live per-launch timing of the dominant kernel: c_fc forward contraction (EPI_QUICKGELU_D8), M = b*S, N = 4D, K = D
        ops.KERNEL_PROBE["gemm_nt"] = {"events": [], "match": lambda epi, M, N, K: epi == ops.EPI_QUICKGELU_D8 and M == Mrows}
    if use_dist:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        loss = one_step(args.warmup + i)
    if use_dist:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    events = ops.KERNEL_PROBE.pop("gemm_nt")["events"] if args.full else []
    if use_dist:
        tmax = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = float(tmax)
    ms = dt / args.steps * 1e3
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, mon.model, loss)
    if args.full:
        live_ms = sum(e0.elapsed_time(e1) for e0, e1 in events) / max(len(events), 1)
        # The roofline figure of the dominant kernel comes from a short SERIAL post-pass (outside the timed region): the same step with
        # the frozen image tower on the main stream, so that the HIP events around a c_fc launch bracket that launch and nothing else --
        # the condition the committed rocprofv3 per-shape tables are taken under (profiles/*_kernel_shapes_serial.txt).  In the timed
        # steps the image tower's launches on the side stream share the chip with the bracketed launch: that number stays as `in_step_*`.
        overlap_was = os.environ.get("VIPANT_TOWER_OVERLAP")
        os.environ["VIPANT_TOWER_OVERLAP"] = "0"
        ops.KERNEL_PROBE["gemm_nt"] = {"events": [], "match": lambda epi, M, N, K: epi == ops.EPI_QUICKGELU_D8 and M == Mrows}
        for i in range(3):
            one_step(args.warmup + args.steps + i)
        torch.cuda.synchronize()
        serial_events = ops.KERNEL_PROBE.pop("gemm_nt")["events"]
        if overlap_was is None:
            del os.environ["VIPANT_TOWER_OVERLAP"]
        else:
            os.environ["VIPANT_TOWER_OVERLAP"] = overlap_was
        serial_events = serial_events[len(serial_events) // 3:]          # the first of the three steps settles clocks and caches
        kern_ms = sum(e0.elapsed_time(e1) for e0, e1 in serial_events) / max(len(serial_events), 1)
        kern_flops = 2.0 * Mrows * (4 * W) * W
        achieved = kern_flops / (kern_ms * 1e-3) / 1e12 if kern_ms > 0 else 0.0
        live = kern_flops / (live_ms * 1e-3) / 1e12 if live_ms > 0 else 0.0
    P = S - 1
    lbr = not args.full_last_block
    step_flops = b * (3 * tower_fwd_flops(S, 1024, P, width=W, layers=args.layers, last_block_rows=lbr)
                      + tower_fwd_flops(50, 3072, 49, layers=min(args.layers, 12), last_block_rows=lbr)) + 6.0 * (b * world) ** 2 * E / world
    out = {
        "metric": "audio_text_pairs_per_sec", "value": round(b * world / (ms * 1e-3), 2), "unit": "pairs/s",
        "n_gpus": world, "ranks": world, "rccl": dist.get_backend() if use_dist else None,
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms, 3),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "e4m3 contractions, bf16 elsewhere (NOT the headline precision)" if args.fp8 else "bf16", "data": "synthetic",
        "config": {"workload": f"VA pretrain step, per-GPU batch {b}, {Fq}-bin x {T}-frame spectrograms (S={S}), audio ViT-{'B' if W == 768 else W}/{args.layers}L "
                               "fwd+bwd + frozen CLIP ViT-B/32 image tower fwd + InfoNCE + LARS (BASELINE.json configs[1]; configs[3] at 8 GPUs)",
                   "global_batch": b * world, "tokens_per_sample": int(S), "parallelism": f"dp{world}",
                   "negatives": "global (all-gather)" if world > 1 else "global",
                   "comm_overlap": args.comm_overlap if world > 1 else "none (one replica)",
                   # every feature and gradient is what the full block gives; --full-last-block computes the discarded rows too
                   "last_block": "read-out rows only (dead-row elimination: exact up to bf16 rounding order)" if lbr else "every token"},
        "loss": round(float(loss.detach()), 4),
        "step_tflops": round(step_flops / (ms * 1e-3) / 1e12, 1),
        "step_mfma_frac": round(step_flops / (ms * 1e-3) / 1e12 / PEAK_BF16_TFLOPS, 4),
    }
    if args.full:
        out["roofline"] = {"bound": "mfma", "kernel": "%s (c_fc forward + QuickGELU, M=%d N=%d K=%d)" % (DOMINANT_KERNEL, Mrows, 4 * W, W),
                           "achieved": round(achieved, 1), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
                           "frac": round(achieved / PEAK_BF16_TFLOPS, 4), "traffic": pmc_traffic(Mrows, 4 * W, W), "traffic_source": PMC_FILE,
                           "algorithmic_flops": kern_flops, "algorithmic_bytes": 2.0 * (Mrows * W + 4 * W * W) + 3.0 * Mrows * 4 * W,
                           "launches_timed": len(serial_events), "avg_launch_ms": round(kern_ms, 4),
                           "timing": "HIP events around each launch in a serial post-pass (image tower on the main stream, 2 of 3 extra steps)",
                           "in_step_avg_launch_ms": round(live_ms, 4), "in_step_frac": round(live / PEAK_BF16_TFLOPS, 4),
                           "in_step_launches_timed": len(events)}
    if rank == 0 and args.full:
        # the InfoNCE kernel group alone (loss + all three gradients) at the 8-GPU global batch B = 4096
        Bn = 4096
        x1 = torch.nn.functional.normalize(torch.randn(Bn, E, device=dev), dim=-1).requires_grad_()
        x2 = torch.nn.functional.normalize(torch.randn(Bn, E, device=dev), dim=-1).requires_grad_()
        ls = torch.tensor(2.6593, device=dev, requires_grad=True)
        for _ in range(3):
            ops.InfoNCEFn.apply(x1, x2, ls, None, 0, Bn, 1.0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            ops.InfoNCEFn.apply(x1, x2, ls, None, 0, Bn, 1.0)
        e1.record()
        torch.cuda.synchronize()
        nce_ms = e0.elapsed_time(e1) / 10
        out["infonce_alone"] = {"B": Bn, "E": E, "ms": round(nce_ms, 4), "tflops": round(6.0 * Bn * Bn * E / (nce_ms * 1e-3) / 1e12, 1),
                                "note": "loss + dx1 + dx2 + dlogit_scale; the B x B fp32 logits are never stored, the bf16 s.dZ matrix and its transpose "
                                        "(2 x 32 MiB at B = 4096) are, between pass 2 and the gradient contraction"}
        # the same group at the step's own batch on one GPU (row-block kernels up to 768 clips: csrc/infonce.hip)
        Bs = 512
        y1 = torch.nn.functional.normalize(torch.randn(Bs, E, device=dev), dim=-1).requires_grad_()
        y2 = torch.nn.functional.normalize(torch.randn(Bs, E, device=dev), dim=-1).requires_grad_()
        for _ in range(3):
            ops.InfoNCEFn.apply(y1, y2, ls, None, 0, Bs, 1.0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            ops.InfoNCEFn.apply(y1, y2, ls, None, 0, Bs, 1.0)
        e1.record()
        torch.cuda.synchronize()
        out["infonce_alone"]["ms_at_B512"] = round(e0.elapsed_time(e1) / 20, 4)
        # ... and in the form one rank of the 8-GPU step runs: all 4096 x 4096 logits for the loss, gradients for its 512 rows only
        for _ in range(3):
            ops.InfoNCEFn.apply(x1, x2, ls, None, Bn - 512, 512, 1.0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            ops.InfoNCEFn.apply(x1, x2, ls, None, Bn - 512, 512, 1.0)
        e1.record()
        torch.cuda.synchronize()
        out["infonce_alone"]["ms_rank_strip_512_of_4096"] = round(e0.elapsed_time(e1) / 10, 4)
        out["infonce_alone"]["workspace_mb"] = round(_ffi.query("vipant_infonce_workspace_bytes", Bn, E) / 1e6, 1)
        out["infonce_alone"]["workspace_mb_rank_strip"] = round(_ffi.query("vipant_infonce_strip_workspace_bytes", Bn, E, 512) / 1e6, 1)
        if world == 1 and not args.no_encoder_alone:
            # The quantity north_star's 0.40 bar is defined on: the AUDIO ENCODER's forward + backward alone, the headline's 512 clips --
            # no image tower, InfoNCE against fixed unit embeddings (55 us), no optimizer.  Two counts of the same time: the FLOPs the
            # build executes (last block on its read-out rows) and SURVEY.md 8-D4's full-block count (88.9 T at b = 512).
            head, lhead_ = mon.model.audio_head, mon.model.loss_head
            fixed = torch.nn.functional.normalize(torch.randn(b, E, device=dev), dim=-1)
            tuned = [p for p in head.parameters() if p.requires_grad] + [p for p in lhead_.parameters() if p.requires_grad]

            def encoder_only():
                for p in tuned:
                    p.grad = None
                loss_a = lhead_(fixed, head(audios, normalized=lhead_.normalized), None, normalized=lhead_.normalized)
                loss_a.backward(gradient=ops.unit_grad(dev))
            for _ in range(3):
                encoder_only()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(10):
                encoder_only()
            torch.cuda.synchronize()
            enc_ms = (time.perf_counter() - t1) / 10 * 1e3
            ex = 3.0 * b * tower_fwd_flops(S, 1024, P, width=W, layers=args.layers, last_block_rows=lbr)
            d4 = 3.0 * b * tower_fwd_flops(S, 1024, P, width=W, layers=args.layers, last_block_rows=False)
            out["audio_encoder_alone"] = {
                "ms": round(enc_ms, 3), "iterations": 10, "clips": b,
                "flops_executed": ex, "flops_d4": d4,
                "frac_executed": round(ex / (enc_ms * 1e-3) / 1e12 / PEAK_BF16_TFLOPS, 4),
                "frac_d4": round(d4 / (enc_ms * 1e-3) / 1e12 / PEAK_BF16_TFLOPS, 4),
                "note": "audio head forward + backward only (north_star: >= 0.40 of MFMA peak on the audio-encoder forward+backward): no image "
                        "tower, loss against fixed unit embeddings, no LARS; frac_d4 credits SURVEY 8-D4's full last block, which the build "
                        "does not execute; peak = 2500 TFLOP/s dense bf16"}
        if world == 1 and lbr and not args.no_full_last_block_check:
            # transparency: the same build, same box, with the towers' last block evaluated on EVERY token (what the reference
            # computes before its read-out discards all rows but one) -- a short untimed-region extra, never `value`
            for head in (mon.model.audio_head, mon.model.image_head):
                if head is not None and hasattr(head, "encoder"):
                    head.encoder.last_block_rows = False
            for i in range(2):
                one_step(i)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for i in range(6):
                loss_full = one_step(2 + i)
            torch.cuda.synchronize()
            ms_full = (time.perf_counter() - t1) / 6 * 1e3
            out["full_last_block"] = {"ms_per_step": round(ms_full, 3), "value": round(b * world / (ms_full * 1e-3), 2), "unit": "pairs/s", "steps": 6,
                                      "note": "running.last_block_rows=False: the discarded rows of the last block computed too"}
        if world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(args, T, Fq)
    if rank == 0:
        print(json.dumps(out), flush=True)
    if use_dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
