"""Two replicas of a `worker=CVASP +model/loss=ce_va` step with a trainable image tower against one process on the concatenated
batch (MI355X, one GPU shared by the ranks over gloo, as tests/test_barlow_replicas_gpu.py): the loss and the parameters after the
LARS step of every rank equal the one-process values to that file's tolerance, and the loss head sends all of its live operands
through exactly ONE all-gather per step."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

OV = ("+running=siamese worker=CVASP monitor=VASMonitor mode=ddp eval=False num_gpus=1 +model/image=vit_val +model/audio=vit_val "
      "+model/text=dummy +model/loss=ce_va +optimizer=standard +running/audio=default model.image.freeze=False "
      "model.audio.pre_encoder.stride=[16,24] model.image.encoder.layers=2 running.audio.max_len=256 "
      "running.audio.num_mel_bins=64 running.epochs=2 running.synthetic_steps=2 optimizer.warmup_epoch=1").split()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _batch(B):
    g = torch.Generator().manual_seed(78)
    return (torch.randn(B, 512, generator=g), torch.randn(B, 3, 224, 224, generator=g), torch.randn(B, 3, 224, 224, generator=g),
            torch.randn(B, 1, 256, 64, generator=g))


def _run(rank, world, port, out):
    if world > 1:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from vipant_amd import parallel
        from vipant_amd.config import compose
        from vipant_amd.module import adjust_learning_rate
        from vipant_amd.monitor import VASMonitor
        B = 8
        b = B // world
        cfg = compose(OV + [f"running.batch_size={b}"])
        cfg.rank = 0
        torch.manual_seed(cfg.seed)
        mon = VASMonitor(cfg, lambda *_: None, torch.device("cuda:0"))
        gathers = []
        orig = parallel._AllGatherRows.apply
        parallel._AllGatherRows.apply = staticmethod(lambda x: (gathers.append(tuple(x.shape)), orig(x))[1])
        sl = slice(rank * b, (rank + 1) * b)
        prime, v1, v2, a1 = (t[sl].cuda() for t in _batch(B))
        adjust_learning_rate(cfg.optimizer, mon.optimizer, mon.dataloader, 1)
        loss = mon.step(prime, v1, v2, a1, None)
        torch.cuda.synchronize()
        sd = {k: v.detach().cpu() for k, v in mon.model.named_parameters() if v.requires_grad}
        torch.save({"loss": float(loss.detach()), "params": sd, "gathers": gathers, "stats": mon.model.report(nstep=1)}, f"{out}.{rank}")
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_replicas_match_single_process_ce_va(tmp_path):
    one, two = str(tmp_path / "one.pt"), str(tmp_path / "two.pt")
    mp.spawn(_run, args=(1, 0, one), nprocs=1, join=True)
    mp.spawn(_run, args=(2, _free_port(), two), nprocs=2, join=True)
    a = torch.load(one + ".0")
    assert a["gathers"] == []
    for r in (0, 1):
        b = torch.load(f"{two}.{r}")
        assert b["gathers"] == [(4, 4 * 512)], b["gathers"]          # prime, view 1, audio, view 2 in ONE collective
        assert abs(a["loss"] - b["loss"]) <= 1e-5 * max(1.0, abs(a["loss"])), (r, a["loss"], b["loss"])
        assert a["stats"] == b["stats"], (a["stats"], b["stats"])
        assert a["params"].keys() == b["params"].keys()
        assert any(k.startswith("image_head.encoder.") for k in a["params"]) and len([k for k in a["params"] if k.startswith("loss_head.")]) == 3
        for k in a["params"]:
            pa, pb = a["params"][k], b["params"][k]
            err = float((pa - pb).abs().max())
            assert err <= 1e-6 + 2e-4 * float(pa.abs().max()), (r, k, err)
