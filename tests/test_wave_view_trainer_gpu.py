"""ASMonitor with the reference's waveform transforms (`running.clf=False running.audio.transform_audio=True
running.audio.audio_transforms=[...]`): a training step is, bit for bit, the hand composition draw_views -> fbank(view=) -> model
from the same generator state; it differs from the step with `transform_audio=False` (before this path existed the two were equal:
the keys were accepted and nothing read them); and the mixup step of `running.clf=True` is the call it always was.
Geometry of tests/test_tagging_trainer_gpu.py: a 2-block tower, T = 256, F = 64, 8 one-second clips of 12 classes."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
OV = ("+running=audioset worker=ASClassifier monitor=ASMonitor +model/audio=vit_val +model/image=vit_val "
      "+model/text=transformer_val +model/loss=bce +optimizer=standard +running/audio=default num_gpus=1 "
      "model.audio.pre_encoder.stride=[16,24] model.image.encoder.layers=2 model.text.encoder.layers=2 "
      "running.audio.max_len=256 running.audio.num_mel_bins=64 running.audio.norms=[-4.94,5.76] running.batch_size=8 running.epochs=1 "
      "running.synthetic_steps=2 running.synthetic_classes=12 running.synthetic_seconds=1.0 running.peep_rate=1 "
      "optimizer.warmup_epoch=1 running.clip_model_root=/nonexistent eval=False")
CHAIN = "running.audio.audio_transforms=[[RandomScale,[1.25]],[RandomNoise,[10,120,0.25]]]"


def _monitor(extra, tmp_path):
    from vipant_amd.config import compose
    from vipant_amd.monitor import ASMonitor
    cfg = compose((OV + " " + extra + f" alias_root={tmp_path} model_name=t").split())
    cfg.rank = 0
    torch.manual_seed(cfg.seed)
    return ASMonitor(cfg, lambda m: None, DEV)


def test_a_transformed_step_is_the_hand_composition_and_differs_from_the_plain_one(tmp_path):
    from vipant_amd.frontend import KaldiFbank
    mon = _monitor(f"running.clf=False running.audio.transform_audio=True {CHAIN}", tmp_path)
    images, wave, nsamples, labels, _ = next(iter(mon.dataloader))
    assert wave.shape == (8, 16000)
    g = mon._aug_generator()
    fb = KaldiFbank.from_config(mon.cfg.running.audio, 16000.0, train=True, device=DEV)
    assert list(fb.chain) == ["RandomScale", "RandomNoise"] and fb.crop_len == 41760
    view = fb.draw_views(8, g)
    assert bool((view[0][:, 1] != 1).all()) and bool(((view[0][:, 1] >= 0.8) & (view[0][:, 1] <= 1.25)).all())
    masks = fb.draw_masks(8, g)
    audios = fb(wave.to(DEV), nsamples.to(DEV), masks=masks, view=view)
    assert audios.shape == (8, 1, 256, 64) and bool(torch.isfinite(audios).all())
    want = mon.model(images.to(DEV), audios, labels.to(DEV))
    inputs, n = mon._step_inputs(mon.make_batch((images, wave, nsamples, labels, None)))
    loss = mon.step(*inputs)
    torch.cuda.synchronize()
    assert n == 8 and torch.equal(inputs[1], audios) and inputs[2].dtype == torch.int64          # no mixup: the labels stay multi-hot
    assert torch.equal(loss.detach(), want.detach()), (float(loss), float(want))
    # the same batch, the same seeds, transform_audio off
    plain = _monitor(f"running.clf=False running.audio.transform_audio=False {CHAIN}", tmp_path)
    assert plain.frontend(True).chain == {}
    pin, _ = plain._step_inputs(plain.make_batch((images, wave, nsamples, labels, None)))
    assert not torch.equal(pin[1], audios)
    with torch.no_grad():                                                      # one model, the two batches
        assert not torch.equal(plain.model(images.to(DEV), pin[1], labels.to(DEV)), plain.model(images.to(DEV), audios, labels.to(DEV)))
    ploss = plain.step(*pin)
    torch.cuda.synchronize()
    assert not torch.equal(ploss.detach(), want.detach())                      # the first steps of two equally initialised trainers
    # ... which is the plain launch on the untouched clips: the generator gave its draws to the masks alone
    g = plain._aug_generator()
    pfb = plain.frontend(True)
    assert torch.equal(pin[1], pfb(wave.to(DEV), nsamples.to(DEV), masks=pfb.draw_masks(8, g)))
    # evaluation applies no chain and clips no longer than crop_len need no view
    mon.model.train(False)
    efb = mon.frontend(False)
    assert efb.chain == {} and efb.train is False
    assert torch.equal(mon.make_batch((images, wave, nsamples, labels, None))[1], efb(wave.to(DEV), nsamples.to(DEV)))


def test_long_clips_take_the_crop_rule(tmp_path):
    """max_len 64 at one-second clips: 16000 > crop_len = 11040: training draws the window from the trainer's generator,
    evaluation takes the centred one; both through the view path."""
    mon = _monitor("running.clf=False running.audio.max_len=64", tmp_path)
    images, wave, nsamples, labels, _ = next(iter(mon.dataloader))
    fb = mon.frontend(True)
    assert fb.chain == {} and fb.crop_len == 11040
    g = mon._aug_generator()
    view = fb.draw_views(8, g)
    want = fb(wave.to(DEV), nsamples.to(DEV), masks=fb.draw_masks(8, g), view=view)
    got = mon.make_batch((images, wave, nsamples, labels, None))[1]
    assert got.shape == (8, 1, 64, 64) and torch.equal(got, want)
    _, nout = fb.view_wave(wave.to(DEV), nsamples.to(DEV), view)
    assert nout.tolist() == [11040] * 8
    mon.model.train(False)
    efb = mon.frontend(False)
    assert torch.equal(mon.make_batch((images, wave, nsamples, labels, None))[1], efb(wave.to(DEV), nsamples.to(DEV), view=True))
    cut = wave[:, 2480:2480 + 11040].contiguous()                              # stationary synthetic clips: the rule keeps the centred window
    assert torch.equal(efb(wave.to(DEV), nsamples.to(DEV), view=True), efb(cut.to(DEV)))


def test_the_mixup_step_is_the_call_it_was(tmp_path, monkeypatch):
    from vipant_amd import frontend
    mon = _monitor(f"running.clf=True running.mixup_rate=1.0 running.audio.transform_audio=True {CHAIN}", tmp_path)
    images, wave, nsamples, labels, _ = next(iter(mon.dataloader))
    calls = []
    real = frontend.KaldiFbank.__call__

    def spy(self, *a, **k):
        calls.append((a, k))
        return real(self, *a, **k)
    monkeypatch.setattr(frontend.KaldiFbank, "__call__", spy)
    monkeypatch.setattr(frontend.KaldiFbank, "draw_views", lambda *a, **k: pytest.fail("the clf branch drew views"))
    got = mon.make_batch((images, wave, nsamples, labels, None))
    monkeypatch.undo()
    assert len(calls) == 1 and calls[0][1].get("view") is None and calls[0][1]["mix"] is not None
    g = mon._aug_generator()
    fb = mon.frontend(True)
    mix = fb.draw_mixup(8, 1.0, g)
    masks = fb.draw_masks(8, g)
    assert torch.equal(calls[0][1]["mix"][0], mix[0]) and torch.equal(calls[0][1]["mix"][1], mix[1]) and torch.equal(calls[0][1]["masks"], masks)
    assert torch.equal(got[1], fb(wave.to(DEV), nsamples.to(DEV), masks=masks, mix=mix))         # vipant_fbank_mix, as before
    assert torch.equal(got[3], mon.soft_labels(labels.to(DEV), *mix))
