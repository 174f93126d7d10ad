"""Two replicas of a `+model/loss=ce_cls` ESClassifier step against one process on the concatenated batch (MI355X, one GPU shared
by the ranks over gloo, as tests/test_barlow_replicas_gpu.py).  Every rank scores its own rows with gradients scaled by 1 / world;
the head's parameter gradients are partial per rank and join the SUM all-reduce, so the parameters after the LARS step equal the
one-process values and the mean of the ranks' losses (each a mean over its rows) equals the one-process loss."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

OV = ("+running=esc50 worker=ESClassifier monitor=ESCMonitor mode=ddp eval=False num_gpus=1 +model/audio=vit_val "
      "+model/image=vit_val +model/text=transformer_val +model/loss=ce_cls +optimizer=standard +running/audio=default "
      "model.audio.pre_encoder.stride=[16,24] model.image.encoder.layers=2 running.audio.max_len=256 "
      "running.audio.num_mel_bins=64 running.epochs=2 running.synthetic_steps=2 running.synthetic_classes=10 "
      "optimizer.warmup_epoch=1 running.clip_model_root=/nonexistent").split()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _batch(B):
    g = torch.Generator().manual_seed(77)
    return torch.randn(B, 1, 256, 64, generator=g), torch.randint(0, 10, (B,), generator=g)


def _run(rank, world, port, out):
    if world > 1:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from vipant_amd.config import compose
        from vipant_amd.module import adjust_learning_rate
        from vipant_amd.monitor import ESCMonitor
        B = 16
        b = B // world
        cfg = compose(OV + [f"running.batch_size={b}"])
        cfg.rank = 0
        torch.manual_seed(cfg.seed)
        mon = ESCMonitor(cfg, lambda *_: None, torch.device("cuda:0"))
        aud, lab = _batch(B)
        sl = slice(rank * b, (rank + 1) * b)
        _, loader = mon.loader_list[0][0]()
        adjust_learning_rate(cfg.optimizer, mon.optimizer, range(2), 1)
        loss = mon.step(aud[sl].cuda(), lab[sl].cuda())
        torch.cuda.synchronize()
        sd = {k: v.detach().cpu() for k, v in mon.model.named_parameters() if v.requires_grad}
        torch.save({"loss": float(loss.detach()), "params": sd}, f"{out}.{rank}")
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_replicas_match_single_process_ce_cls(tmp_path):
    one, two = str(tmp_path / "one.pt"), str(tmp_path / "two.pt")
    mp.spawn(_run, args=(1, 0, one), nprocs=1, join=True)
    mp.spawn(_run, args=(2, _free_port(), two), nprocs=2, join=True)
    a = torch.load(one + ".0")
    ranks = [torch.load(f"{two}.{r}") for r in (0, 1)]
    mean = sum(b["loss"] for b in ranks) / 2
    assert abs(a["loss"] - mean) <= 1e-5 * max(1.0, abs(a["loss"])), (a["loss"], [b["loss"] for b in ranks])
    for r, b in enumerate(ranks):
        assert a["params"].keys() == b["params"].keys()
        assert any(k.startswith("loss_head.linear") for k in a["params"]) and "loss_head.logit_scale" in a["params"]
        for k in a["params"]:
            pa, pb = a["params"][k], b["params"][k]
            err = float((pa - pb).abs().max())
            assert err <= 1e-6 + 2e-4 * float(pa.abs().max()), (r, k, err)
