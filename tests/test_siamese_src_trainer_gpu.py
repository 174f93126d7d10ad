"""The siamese multi-view trainer from files (`monitor=VASMonitor worker=CVASP +running=siamese +model/loss=ce_va` with
`running.data_root=DIR`): a generated directory in the reference's layout -- 8 clips of 0.02 to 0.9 s, mono and stereo, two of them
longer than crop_len = 0.69 s, PNG frames, frame embeddings for the records that list their frames -- goes through the siamese
loader, `pcm_wave`, the pair launch of the log-mel front-end and the image views; the two audio views the worker sees are, bit for
bit, what the single-call front-end gives for the draws and masks replayed in the documented order from a generator seeded the same
way.  Geometry: one block per tower, resolution 32, T = 64, F = 64, batch 4, 2 steps.  Without `data_root` the trainer is what it
was: the loss strings below come from the parent commit."""
import json
import os
import re
import warnings

import numpy as np
import pytest
import torch

import src_fixture as SF

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
COMMON = ("+model/image=vit_val +model/audio=vit_val +model/text=dummy +optimizer=standard +running/audio=default num_gpus=1 "
          "model.audio.pre_encoder.stride=[16,24] model.image.encoder.layers=1 model.image.resolution=32 running.audio.max_len=64 "
          "running.audio.num_mel_bins=64 running.batch_size=4 running.synthetic_steps=2 optimizer.epochs=1 optimizer.warmup_epoch=1 "
          "running.clip_model_root=/nonexistent")
# `running.siamese.alive=True`: the worker's siamese backbone, which keeps the image tower (the separate backbone destroys it as soon
# as `running.frame_emb` is set, and the siamese src dataset requires that key)
SIAMESE = ("+running=siamese worker=CVASP monitor=VASMonitor +model/loss=ce_va model.image.freeze=False model.loss.aa=True "
           "running.siamese.alive=True " + COMMON)
SECONDS = [0.3, 0.9, 0.5, 0.69, 0.2, 0.8, 0.6, 0.02]
CHANNELS = [1, 2, 1, 2, 2, 1, 2, 1]
FRAMES = [(37, 53), (96, 128), (64, 48), (50, 50), (96, 40), (37, 128), (72, 96), (40, 41)]
NAMES = [0, 2, 0, 5, 1, 0, 6, 3]             # frame names per item: 0 = the frame is a string (no embedding file)
SR, T, F, E = 16000, 64, 64, 512
CROP_LEN = int((T / 100 + 0.05) * SR)        # 11040 samples = 0.69 s
FBANK_NORMS = (-4.93839311, 5.75751113)      # FbankTransform's constants (cvap/data/audio/transform.py:228-229)

# `data_root=""`: the loss strings of the two steps, as printed by the PARENT commit for SIAMESE + " eval=False" on an MI355X (two runs there gave the same strings): nothing
# of this pull request may move them.
PARENT_LOSSES = [("1", "10.459"), ("2", "10.525")]


@pytest.fixture(scope="module")
def src_dir(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("siamese_src"))
    records, clips, frames = SF.make_src_dir(root, "src_train_toy", SECONDS, CHANNELS, FRAMES, nframes_per_item=NAMES,
                                             sub_dirs=["", "bal", "", "bal", "", "", "bal", ""])
    with open(f"{root}/src_eval_toy.csv", "w") as f:
        for r in records:
            f.write(json.dumps(r) + "\n")
    g = np.random.default_rng(9)
    os.makedirs(f"{root}/emb")
    for r, k in zip(records, NAMES):
        for j in range(k):
            np.savez(f"{root}/emb/{r['id']}.{j:03d}.npz", v=g.standard_normal(E).astype(np.float32))
    assert sum(c.shape[0] > CROP_LEN for c in clips) == 2 and clips[3].shape[0] == CROP_LEN
    return root, records, clips, frames


def _monitor(ov, tmp=None):
    from vipant_amd import monitor
    from vipant_amd.config import compose
    if tmp is not None:
        ov += (f" running.data_root={tmp} running.data_name=src_train_toy running.eval_name=src_eval_toy running.frame_emb=emb "
               f"alias_root={tmp}/out")
    cfg = compose(ov.split())
    cfg.rank = 0
    torch.manual_seed(cfg.seed)
    lines = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return monitor.VASMonitor(cfg, lambda m: lines.append(str(m)), DEV), lines


def _losses(lines):
    return re.findall(r"step (\d)\tlr_w \S+ lr_b \S+ loss (\d+\.\d{3})", "\n".join(lines))


def _frontend(train):
    from vipant_amd.frontend import KaldiFbank
    return KaldiFbank(float(SR), F, T, norms=FBANK_NORMS, zero_mean_wf=True, train=train, device=DEV)


def _wave(clips):
    from vipant_amd.frontend import pcm_wave
    return pcm_wave(clips.pcm.to(DEV), clips.nframes, clips.channels, mode="first")


def test_two_steps_from_files_and_the_worker_sees_the_single_calls(src_dir):
    from vipant_amd.data import FrameBatch, PcmBatch, SecondView
    from vipant_amd.image_views import ImageViews
    root = src_dir[0]
    mon, lines = _monitor(SIAMESE + " eval=False", root)
    assert "Instantiate main dataloader from `src_train_toy': total 2 (1) batches." in lines
    assert mon.evalloader is not None and mon.gold_file == f"{root}/src_eval_toy.csv"
    before = {k: p.detach().clone() for k, p in mon.model.named_parameters() if p.requires_grad}
    assert len(before) > 10
    raws, seen = [], []
    real_batch, real_forward = mon.make_batch, mon.model.forward

    def spy_batch(batch):
        if mon.model.training:
            raws.append(batch)
        return real_batch(batch)

    def spy_forward(images, images_v1, audios_v1, **kw):
        if mon.model.training:
            seen.append((images, images_v1, kw.get("images_v2"), audios_v1, kw.get("audios_v2")))
        return real_forward(images, images_v1, audios_v1, **kw)
    mon.make_batch, mon.model.forward = spy_batch, spy_forward
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                # (a record with a single frame name: the warned random embedding)
        mon.learn()
    torch.cuda.synchronize()
    steps = _losses(lines)
    assert [int(s[0]) for s in steps] == [1, 2] and all(np.isfinite(float(s[1])) for s in steps), lines
    assert len(raws) == len(seen) == 2
    still = [k for k, p in mon.model.named_parameters() if p.requires_grad and torch.equal(p.detach(), before[k])]
    assert not still, still
    # by hand: the documented draw order, from a generator seeded the same way and consumed in step order
    g = torch.Generator().manual_seed(int(mon.cfg.seed) + 7 + 1000 * 0)
    gi = mon._image_views_generator()
    fb = _frontend(True)
    assert fb.crop_len == CROP_LEN
    prime = ImageViews.from_config(mon.cfg.running, True, "prime", device=DEV, siamese=True)
    second = ImageViews.from_config(mon.cfg.running, True, "second", device=DEV, siamese=True)
    views = 0
    for raw, (images, images_v1, images_v2, audios_v1, audios_v2) in zip(raws, seen):
        assert isinstance(raw[1], FrameBatch) and isinstance(raw[3], PcmBatch) and raw[3].pcm.device.type == "cpu"
        assert isinstance(raw[2], SecondView) and isinstance(raw[4], SecondView)
        assert images.shape == (4, E) and torch.equal(images.cpu(), raw[0])
        wave, nsamples = _wave(raw[3])
        crop = int(raw[3].nframes.max()) > CROP_LEN
        views += crop
        view = fb.draw_views(4, g) if crop else fb.no_views(4)
        m1 = fb.draw_masks(4, g, freq_mask_param=32, time_mask_param=200)
        m2 = fb.draw_masks(4, g, freq_mask_param=48, time_mask_param=300)
        assert audios_v1.shape == audios_v2.shape == (4, 1, T, F) and audios_v1.dtype == torch.float32
        assert torch.equal(audios_v1, fb(wave, nsamples, masks=m1, view=view))
        assert torch.equal(audios_v2, fb(wave, nsamples, masks=m2, view=view))
        assert bool(torch.isfinite(audios_v1).all()) and bool(torch.isfinite(audios_v2).all())
        frames, hw = raw[1].frames.to(DEV), raw[1].hw
        assert torch.equal(images_v1, prime(frames, hw=hw, draws=prime.draw_image_views(hw, gi)))
        assert torch.equal(images_v2, second(frames, hw=hw, draws=second.draw_image_views(hw, gi)))
    assert views >= 1                                  # two of the eight clips are longer than crop_len: some batch crops
    # evaluation: the centred crop, FbankTransform's constants, no masks, no second view, no draw
    mon.make_batch, mon.model.forward = real_batch, real_forward
    mon.model.train(False)
    state = g.get_state()
    ev = _frontend(False)
    for raw in raws:
        e = mon.make_batch(raw)
        wave, nsamples = _wave(raw[3])
        assert e[4] is None and torch.equal(e[3], ev(wave, nsamples, view=True))
    assert torch.equal(mon.aug_generator.get_state(), state)      # (and training left the trainer's generator where the replay's is)


def test_without_aa_there_is_no_second_view(src_dir):
    root = src_dir[0]
    mon, _ = _monitor(SIAMESE + " eval=False model.loss.aa=False", root)
    raw = next(iter(mon.dataloader))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        batch = mon.make_batch(raw)
    assert batch[4] is None
    g = torch.Generator().manual_seed(int(mon.cfg.seed) + 7 + 1000 * 0)
    fb = _frontend(True)
    wave, nsamples = _wave(raw[3])
    view = fb.draw_views(4, g) if int(raw[3].nframes.max()) > CROP_LEN else fb.no_views(4)
    m1 = fb.draw_masks(4, g, freq_mask_param=32, time_mask_param=200)
    assert torch.equal(batch[3], fb(wave, nsamples, masks=m1, view=view))
    assert torch.equal(mon.aug_generator.get_state(), g.get_state())           # no second set was drawn


def test_eval_norms_is_refused_under_multi_view(src_dir):
    from vipant_amd._ffi import VipantError
    with pytest.raises(VipantError, match="eval_norms under running.multi_view"):
        _monitor(SIAMESE + " eval=False running.audio.eval_norms=True", src_dir[0])


def test_without_data_root_the_trainer_is_the_parent_s():
    mon, lines = _monitor(SIAMESE + " eval=False")
    assert "Instantiate main dataloader from `synthetic': total 2 batches." in lines
    mon.learn()
    torch.cuda.synchronize()
    assert _losses(lines) == PARENT_LOSSES, lines
