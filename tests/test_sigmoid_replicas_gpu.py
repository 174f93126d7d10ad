"""Two replicas of SigmoidLossHead with global negatives (one GPU shared over gloo, fresh child processes) against one process on the
concatenated batch: loss, each half's feature gradients, both parameter gradients; bounds of tests/test_replicas_gpu.py."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
B = 48


def _run(rank, world, port, out):
    if world > 1:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from test_sigmoid_head_gpu import build_head, features, step
        x1, x2 = (3.0 * v for v in features(B, 512))
        sl = slice(rank * (B // world), (rank + 1) * (B // world))
        res = step(build_head(negatives="global"), x1[sl], x2[sl])
        torch.save({k: v.cpu() for k, v in res.items()}, f"{out}.{rank}")
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_two_replicas_match_single_process_sigmoid(tmp_path):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_run, args=(1, 0, str(tmp_path / "one")), nprocs=1, join=True)
    mp.spawn(_run, args=(2, port, str(tmp_path / "two")), nprocs=2, join=True)
    a = torch.load(tmp_path / "one.0")
    for r in (0, 1):
        t = torch.load(tmp_path / f"two.{r}")
        assert abs(float(a["loss"] - t["loss"])) <= 1e-5 * max(1.0, abs(float(a["loss"]))), (r, a["loss"], t["loss"])
        for k in ("dx1", "dx2", "dls", "dlb"):
            want = a[k][r * B // 2:(r + 1) * B // 2] if k.startswith("dx") else a[k]
            assert float((want - t[k]).abs().max()) <= 1e-6 + 2e-4 * float(want.abs().max()), (r, k)
