"""The trainers from decoded frames (`running.image_frames=[48, 64]`): the siamese trainer turns one uint8 frame batch into the prime and
the second `barlow` view, the bimodal trainer into the `clip` view, and what the worker sees is, bit for bit, the direct `ImageViews`
call with the same generator.  Without the key the batches -- and with them the loss sequence -- are what they were.
Geometry: 2-block towers, resolution 32 (one 32-pixel patch), T = 256, F = 64, batch 4, 2 steps."""
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
COMMON = ("+model/image=vit_val +model/audio=vit_val +model/text=dummy +optimizer=standard +running/audio=default num_gpus=1 eval=False "
          "model.audio.pre_encoder.stride=[16,24] model.image.encoder.layers=2 model.image.resolution=32 running.audio.max_len=256 "
          "running.audio.num_mel_bins=64 running.batch_size=4 running.synthetic_steps=2 optimizer.epochs=1 optimizer.warmup_epoch=1 "
          "running.clip_model_root=/nonexistent")
SIAMESE = "+running=siamese worker=CVASP monitor=VASMonitor +model/loss=ce_va model.image.freeze=False " + COMMON
BIMODAL = "+running=bimodal worker=CVALP monitor=VAMonitor +model/loss=ce model.image.freeze=False " + COMMON
KEY = " +running.image_frames=[48,64]"


def _monitor(ov, name):
    from vipant_amd import monitor
    from vipant_amd.config import compose
    cfg = compose(ov.split())
    cfg.rank = 0
    torch.manual_seed(cfg.seed)
    lines = []
    return getattr(monitor, name)(cfg, lambda m: lines.append(str(m)), DEV), lines


def _losses(lines):
    return re.findall(r"step (\d)\tlr_w \S+ lr_b \S+ loss (\d+\.\d{3})", "\n".join(lines))


def test_siamese_trainer_runs_from_uint8_frames():
    from vipant_amd.image_views import ImageViews
    mon, lines = _monitor(SIAMESE + KEY, "VASMonitor")
    raw = next(iter(mon.dataloader))
    assert raw[1].dtype == torch.uint8 and raw[1].shape == (4, 48, 64, 3) and raw[2] is raw[1]
    g = mon._image_views_generator()
    prime = ImageViews.from_config(mon.cfg.running, True, "prime", device=DEV)
    second = ImageViews.from_config(mon.cfg.running, True, "second", device=DEV)
    assert (prime.chain, second.chain, prime.n_px) == ("barlow", "barlow", 32)
    frames = raw[1].to(DEV)
    want1 = prime(frames, draws=prime.draw_image_views([[48, 64]] * 4, g))
    want2 = second(frames, draws=second.draw_image_views([[48, 64]] * 4, g))
    seen = []
    real = mon.model.forward

    def spy(images, images_v1, audios_v1, **kw):
        seen.append((images_v1, kw.get("images_v2")))
        return real(images, images_v1, audios_v1, **kw)
    mon.model.forward = spy
    mon.learn()
    torch.cuda.synchronize()
    assert len(seen) == 2 and seen[0][0].shape == (4, 3, 32, 32) and seen[0][0].dtype == torch.float32
    assert torch.equal(seen[0][0], want1) and torch.equal(seen[0][1], want2)            # the worker's views are the direct calls
    assert not torch.equal(want1, want2) and bool(torch.isfinite(seen[1][0]).all())
    steps = _losses(lines)
    assert [int(s[0]) for s in steps] == [1, 2] and all(float(s[1]) == float(s[1]) for s in steps), lines
    # the second view is built only when model.loss.vv reads it; evaluation and clip_tf take the clip chain
    off, _ = _monitor(SIAMESE + KEY + " model.loss.vv=False", "VASMonitor")
    batch = off.make_batch(raw)
    assert batch[2] is None and torch.equal(batch[1], want1)
    tf, _ = _monitor(SIAMESE + KEY + " running.clip_tf=True", "VASMonitor")
    clip = ImageViews(32, "clip", device=DEV)(frames)
    b = tf.make_batch(raw)
    assert torch.equal(b[1], clip) and torch.equal(b[2], clip)
    mon.model.train(False)
    e = mon.make_batch(raw)
    assert torch.equal(e[1], clip)


def test_bimodal_trainer_runs_from_uint8_frames():
    from vipant_amd.image_views import ImageViews
    mon, lines = _monitor(BIMODAL + KEY, "VAMonitor")
    raw = next(iter(mon.dataloader))
    assert raw[0].dtype == torch.uint8 and raw[0].shape == (4, 48, 64, 3)
    images = mon.make_batch(raw)[0]
    assert torch.equal(images, ImageViews(32, "clip", device=DEV)(raw[0].to(DEV)))
    mon.learn()
    torch.cuda.synchronize()
    assert [int(s[0]) for s in _losses(lines)] == [1, 2], lines


def test_without_the_key_nothing_changes(monkeypatch):
    """The loss sequence of a run that never hears of frames: no ImageViews is built, the batches are the loader's float tensors, and
    two such runs print the same losses (the run with the key prints others)."""
    from vipant_amd import image_views
    built = []
    real = image_views.ImageViews.__init__
    monkeypatch.setattr(image_views.ImageViews, "__init__", lambda self, *a, **k: (built.append(1), real(self, *a, **k))[1])
    mon, lines = _monitor(SIAMESE, "VASMonitor")
    raw = next(iter(mon.dataloader))
    assert raw[1].dtype == torch.float32 and raw[1].shape == (4, 3, 32, 32)
    batch = mon.make_batch(raw)
    assert torch.equal(batch[1], raw[1].to(DEV)) and torch.equal(batch[2], raw[2].to(DEV))
    mon.learn()
    again, lines2 = _monitor(SIAMESE, "VASMonitor")
    again.learn()
    torch.cuda.synchronize()
    assert not built
    assert len(_losses(lines)) == 2 and _losses(lines) == _losses(lines2)
    keyed, lines3 = _monitor(SIAMESE + KEY, "VASMonitor")
    keyed.learn()
    torch.cuda.synchronize()
    assert built and _losses(lines3) != _losses(lines)
