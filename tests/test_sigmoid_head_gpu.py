"""SigmoidLossHead through the public interface: the composed `+model/loss=sigmoid` group against float64 autograd through normalise +
loss (loss 1e-3, gradients by the rules of tests/test_sigmoid_loss_gpu.py), local negatives, the evaluation report, two trainer steps."""
import math

import pytest
import torch

import vipant_amd.module as M
from test_sigmoid_loss_gpu import close, features, reference
from vipant_amd.config import compose, to_config
from vipant_amd.monitor import VAMonitor

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OV = ("+running=bimodal worker=CVALP mode=dp eval=False num_gpus=1 +model/image=vit_val +model/audio=vit_val +model/text=dummy "
      "+model/loss=sigmoid +optimizer=standard +running/audio=default model.audio.pre_encoder.stride=[16,24] model.image.encoder.layers=1 "
      "running.audio.max_len=256 running.audio.num_mel_bins=64 running.batch_size=16 running.epochs=2 running.frame_emb=synthetic "
      "running.synthetic_steps=2 running.save_epoch=False optimizer.warmup_epoch=1").split()


def build_head(**kwargs):
    return M.build_loss_head(compose(OV).model.loss, **kwargs).to(DEV)


def step(head, x1, x2):
    a1, a2 = x1.clone().requires_grad_(), x2.clone().requires_grad_()
    loss = head.train()(a1, a2, None, normalized=False)
    loss.backward()
    return {"loss": loss.detach(), "dx1": a1.grad, "dx2": a2.grad, "dls": head.logit_scale.grad, "dlb": head.logit_bias.grad}


@pytest.mark.parametrize("B", [8, 48])
def test_head_against_fp64_autograd(B):
    """also: the state dict round trip; local negatives in one process give the plain call's bits; the report is CELossHead's string"""
    x1, x2 = (3.0 * v for v in features(B, 512))          # un-normalised: the head normalises
    head, local = build_head(), build_head(negatives="local")
    assert type(head).__name__ == "SigmoidLossHead" and sorted(head.state_dict()) == ["logit_bias", "logit_scale"]
    local.copy_state_dict({"logit_scale": torch.tensor(1.5), "logit_bias": torch.tensor(-3.0), "unrelated": torch.zeros(2)})
    assert float(local.logit_scale.detach()) == 1.5 and float(local.logit_bias.detach()) == -3.0
    local.copy_state_dict(head.state_dict())
    got, same = step(head, x1, x2), step(local, x1, x2)
    assert all(torch.equal(got[k], same[k]) for k in got)
    r1, r2 = x1.double().requires_grad_(), x2.double().requires_grad_()
    ls, lb = (p.detach().double().clone().requires_grad_() for p in (head.logit_scale, head.logit_bias))
    n1, n2 = torch.nn.functional.normalize(r1, dim=-1), torch.nn.functional.normalize(r2, dim=-1)
    ref = reference(n1, n2, ls, lb)["loss"]
    want = dict(zip(("dx1", "dx2", "dls", "dlb"), torch.autograd.grad(ref, [r1, r2, ls, lb], retain_graph=True)))
    emu = reference(n1.detach(), n2.detach(), ls.detach(), lb.detach(), emulate=True)      # then float64 through the normalisation
    emu["dx1"], emu["dx2"] = torch.autograd.grad([n1, n2], [r1, r2], [emu["dx1"], emu["dx2"]])
    bad = [k for k in want if not close(k, got[k], want[k], emu[k])]
    assert not bad and abs(float(got["loss"]) - float(ref)) <= 1e-3, (bad, float(got["loss"]), float(ref))
    ce = M.build_loss_head(to_config({"name": "CELossHead", "layers": [], "scaling": True, "scale_max": None})).to(DEV)
    with torch.no_grad():
        for h in (head, ce):
            h.eval()(x1, x2, normalized=False)
    want = ce.report()
    assert want.endswith(f"@ {B}") and head.report() == want


def test_two_trainer_steps():
    cfg = compose(OV)
    cfg.rank = 0
    torch.manual_seed(cfg.seed)
    mon = VAMonitor(cfg, lambda *_: None, torch.device(DEV))
    head, losses = mon.model.loss_head, []
    assert {id(head.logit_scale), id(head.logit_bias)} <= {id(p) for p in mon.params}
    for step, batch in enumerate(mon.dataloader):
        images, audios, _, _, _ = mon.make_batch(batch)
        M.adjust_learning_rate(cfg.optimizer, mon.optimizer, mon.dataloader, step + 1)
        losses.append(float(mon.step(images, audios, None)))
    # the two steps see different synthetic batches, so the loss need not fall; it must not leave the scale it started at
    assert len(losses) == 2 and all(math.isfinite(v) for v in losses) and 0.0 < losses[1] <= 2.0 * losses[0], losses
    assert math.isfinite(float(head.logit_scale.detach())) and math.isfinite(float(head.logit_bias.grad))
