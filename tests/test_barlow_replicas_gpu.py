"""Two replicas of a `+model/loss=barlow_ce` VA step against one process on the concatenated batch (MI355X, one GPU shared by
the ranks over gloo, as tests/test_replicas_gpu.py).  Every rank runs the projector, the batch norms and c over the all-gathered
batch, so the loss, the parameters after the LARS step and the running statistics of every rank equal the one-process values."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

OV = ("+running=bimodal worker=CVALP mode=ddp eval=False num_gpus=1 +model/image=vit_val +model/audio=vit_val "
      "+model/text=dummy +model/loss=barlow_ce +optimizer=standard +running/audio=default "
      "model.audio.pre_encoder.stride=[16,24] model.image.encoder.layers=2 running.audio.max_len=256 "
      "running.audio.num_mel_bins=64 running.epochs=2 running.frame_emb=synthetic "
      "running.synthetic_steps=2 running.save_epoch=False optimizer.warmup_epoch=1 "
      "model.loss.barlow.layers=[256,512,512]").split()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _batch(B):
    g = torch.Generator().manual_seed(77)
    return torch.randn(B, 512, generator=g), torch.randn(B, 1, 256, 64, generator=g)


def _run(rank, world, port, out):
    if world > 1:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from vipant_amd.config import compose
        from vipant_amd.module import adjust_learning_rate
        from vipant_amd.monitor import VAMonitor
        B = 16
        b = B // world
        cfg = compose(OV + [f"running.batch_size={b}"])
        cfg.rank = 0
        torch.manual_seed(cfg.seed)
        mon = VAMonitor(cfg, lambda *_: None, torch.device("cuda:0"))
        img, aud = _batch(B)
        sl = slice(rank * b, (rank + 1) * b)
        adjust_learning_rate(cfg.optimizer, mon.optimizer, mon.dataloader, 1)
        loss = mon.step(img[sl].cuda(), aud[sl].cuda(), None)
        torch.cuda.synchronize()
        sd = {k: v.detach().cpu() for k, v in mon.model.named_parameters() if v.requires_grad}
        bufs = {k: v.detach().cpu() for k, v in mon.model.loss_head.named_buffers()}
        torch.save({"loss": float(loss.detach()), "params": sd, "buffers": bufs}, f"{out}.{rank}")
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_replicas_match_single_process_barlow_ce(tmp_path):
    one, two = str(tmp_path / "one.pt"), str(tmp_path / "two.pt")
    mp.spawn(_run, args=(1, 0, one), nprocs=1, join=True)
    mp.spawn(_run, args=(2, _free_port(), two), nprocs=2, join=True)
    a = torch.load(one + ".0")
    for r in (0, 1):
        b = torch.load(f"{two}.{r}")
        assert abs(a["loss"] - b["loss"]) <= 1e-5 * max(1.0, abs(a["loss"])), (r, a["loss"], b["loss"])
        assert a["params"].keys() == b["params"].keys()
        assert any(k.startswith("loss_head.loss_barlow.linear") for k in a["params"])
        for k in a["params"]:
            pa, pb = a["params"][k], b["params"][k]
            err = float((pa - pb).abs().max())
            assert err <= 1e-6 + 2e-4 * float(pa.abs().max()), (r, k, err)
        for k in a["buffers"]:
            ba, bb = a["buffers"][k], b["buffers"][k]
            if k.endswith("num_batches_tracked"):
                assert int(ba) == int(bb) == 2, k
            else:
                assert float((ba - bb).abs().max()) <= 1e-5 * float(ba.abs().max()) + 1e-7, (r, k)
