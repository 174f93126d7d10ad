"""The two classification trainers from files on the MI355X: `monitor=ESCMonitor running.data_root=DIR` over a toy ESC-50 directory and
`monitor=ASMonitor running.data_root=DIR` over a toy AudioSet directory (tests/clf_fixture.py), through the datasets of
vipant_amd/data/classify.py, `pcm_wave`, the log-mel front-end and 1-block towers (T = 128, F = 64, 16 kHz clips of at most 1 s, batches
of 4).  What a trainer's `make_batch` yields is, bit for bit, the direct calls with a generator seeded the same way: for the tagging
trainer `KaldiFbank(mix=, outputs=)` over the collated b + p rows and `ASMonitor.soft_labels` on the dense multi-hot rows.  With
`running.data_root` empty both trainers still build their synthetic loaders."""
import math
import re

import numpy as np
import pytest
import torch

import clf_fixture as CF

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SR, T, F = 16000, 128, 64
COMMON = ("+model/audio=vit_val +model/image=vit_val +model/text=transformer_val +optimizer=standard +running/audio=default num_gpus=1 "
          "model.audio.pre_encoder.stride=[16,24] model.image.encoder.layers=1 model.text.encoder.layers=1 "
          f"running.audio.max_len={T} running.audio.num_mel_bins={F} running.batch_size=4 running.epochs=1 running.synthetic_steps=2 "
          "running.peep_rate=1 optimizer.warmup_epoch=1 running.clip_model_root=/nonexistent")
ESC = "+running=esc50 worker=ESClassifier monitor=ESCMonitor +model/loss=ce_cls running.synthetic_classes=8 " + COMMON
TAG = ("+running=audioset worker=ASClassifier monitor=ASMonitor +model/loss=bce running.audio.norms=[-4.94,5.76] "
       "running.synthetic_classes=12 running.synthetic_seconds=1.0 " + COMMON)
CLASSES = ["/m/0a", "/m/0b", "/m/0c", "/m/0e", "/m/0h"]


def _monitor(kind, ov, root=None, extra=()):
    from vipant_amd import monitor
    from vipant_amd.config import compose
    if root is not None:
        ov += f" running.data_root={root} running.bpe_path={CF.BPE} alias_root={root}/out model_name=t"
    cfg = compose(ov.split() + list(extra))                 # `extra`: overrides whose value holds blanks
    cfg.rank = 0
    torch.manual_seed(cfg.seed)
    lines = []
    return getattr(monitor, kind)(cfg, lambda m: lines.append(str(m)), DEV), lines


@pytest.fixture(scope="module")
def esc_dir(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("esc"))
    clips = CF.make_esc50_dir(root, ensemble=True)
    assert max(c.shape[0] for c in clips.values()) <= SR and {c.shape[1] for c in clips.values()} == {1, 2}
    return root, clips


@pytest.fixture(scope="module")
def tag_dir(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("tag"))
    records = [{"id": f"t{i}", "dir": "bal" if i % 3 == 0 else "", "clip": ["wav"], "frame": "png",
                "labels": [CLASSES[i % 5]] + ([CLASSES[(i + 2) % 5], CLASSES[i % 5]] if i % 2 else [])} for i in range(8)]
    records, clips = CF.make_audioset_dir(root, name="src_train_toy", records=records, seconds=(0.5, 0.31, 1.0, 0.42, 0.27), channels=(1, 2))
    CF.make_audioset_dir(root, name="src_eval_toy", records=records[:4], seconds=(0.5, 0.31, 1.0, 0.42, 0.27), channels=(1, 2))
    return root, records, clips


# ------------------------------------------------------------------ 1. ESCMonitor from a toy ESC-50 directory
def test_esc_make_batch_is_the_direct_front_end_call(esc_dir):
    from vipant_amd.data import PcmBatch
    from vipant_amd.frontend import KaldiFbank, pcm_wave
    root, clips = esc_dir
    # tile_audio is ON in the configuration: the x-fold trainer must not tile all the same (esc50.py:81)
    mon, lines = _monitor("ESCMonitor", ESC + " eval=False running.audio.tile_audio=True", root, extra=["running.prompt=the sound of"])
    assert "Instantiate 5-fold dataloaders from `esc50': 5 classes." in lines and len(mon.loader_list) == 5
    assert mon.lid2str == {int(k): v for k, v in CF.GOLD["esc50"]["cases"][0]["lid2str"].items()}
    assert np.asarray(mon.lid2int).tolist() == CF.GOLD["esc50"]["cases"][0]["lid2int"] and mon.label_map == {i: i for i in range(5)}
    _, loader = mon.loader_list[1][0]()
    raw = next(iter(loader))
    assert isinstance(raw[0], PcmBatch) and raw[0].pcm.device.type == "cpu" and raw[1].dtype == torch.int64 and len(raw[2]) == 4
    audios, labels, names = mon.make_batch(raw)
    g = torch.Generator().manual_seed(int(mon.cfg.seed) + 7 + 1000 * 0)
    fb = KaldiFbank.from_config(mon.cfg.running.audio, float(SR), train=True, device=DEV)
    assert (fb.freq_mask_param, fb.time_mask_param, fb.chain) == (32, 200, {}) and int(raw[0].nframes.max()) < fb.crop_len
    wave, nsamples = pcm_wave(raw[0].pcm.to(DEV), raw[0].nframes, raw[0].channels, mode="first")
    assert nsamples.tolist() == raw[0].nframes.tolist()                                # not tiled to max_len
    want = fb(wave, nsamples, masks=fb.draw_masks(4, g), view=None)
    assert audios.shape == (4, 1, T, F) and audios.dtype == torch.float32 and torch.equal(audios, want)
    assert labels.is_cuda and torch.equal(labels.cpu(), raw[1]) and names == raw[2]
    assert names == [mon.lid2str[int(k)] for k in raw[1]]
    # evaluation: no masks, nothing drawn
    mon.model.eval()
    _, loader = mon.loader_list[1][1]()
    raw = next(iter(loader))
    audios, labels, _ = mon.make_batch(raw)
    fe = KaldiFbank.from_config(mon.cfg.running.audio, float(SR), train=False, device=DEV)
    wave, nsamples = pcm_wave(raw[0].pcm.to(DEV), raw[0].nframes, raw[0].channels, mode="first")
    assert audios.shape == (2, 1, T, F) and torch.equal(audios, fe(wave, nsamples))
    held = [r["aclip"] for r in CF.GOLD["esc50"]["cases"][0]["folds"][1]["eval"]]
    assert raw[0].nframes.tolist() == [clips[a].shape[0] for a in held]


def test_esc_one_epoch_on_each_of_the_five_folds(esc_dir):
    root, _ = esc_dir
    mon, lines = _monitor("ESCMonitor", ESC + " eval=False", root, extra=["running.prompt=the sound of"])
    mon.learn()
    torch.cuda.synchronize()
    text = "\n".join(lines)
    assert text.count("Training started") == 5 and "Total 1 epochs for each of 5 folds." in text, text
    assert re.search(r"Best mean and std: \d+\.\d\d \\pm \d+\.\d\d in the 0th epoch\.", text), text
    losses = [float(m) for m in re.findall(r"loss (\d+\.\d+) ", text)]
    assert len(losses) == 10 and all(math.isfinite(x) for x in losses), text         # 8 training clips a fold: two steps of 4
    assert len(re.findall(r"A->T: p1 = \d+\.\d\d @ 2", text)) == 5                    # the held-out fold: 2 clips
    assert len(mon.report_by_fold) == 5 and all(len(r) == 1 for r in mon.report_by_fold)


@pytest.mark.parametrize("prompt", ["the sound of", "ensemble"])
def test_esc_zero_shot_on_real_prompts(esc_dir, prompt):
    root, _ = esc_dir
    mon, lines = _monitor("ESCMonitor", ESC + " eval=True running.zero_shot=True", root, extra=[f"running.prompt={prompt}"])
    case = CF.GOLD["esc50"]["cases"][0 if prompt == "the sound of" else 2]
    assert np.asarray(mon.lid2int).tolist() == case["lid2int"] and f"{case['prompts']}" in lines
    seen = {}
    head = mon.model.loss_head
    real_report = head.report

    def spy_report(gold_file=None, **kw):
        seen.update(audios=torch.cat(head.audios).float().cpu(), gold=torch.cat(head.x2s).cpu(), text=kw["text"].float().cpu(),
                    label_map=kw.get("label_map", None))
        return real_report(gold_file=gold_file, **kw)
    head.report = spy_report
    mon.learn()
    torch.cuda.synchronize()
    text = "\n".join(lines)
    assert "(Zero-shot) Evaluating started..." in text and re.search(r"\d+\.\d\d for zero-shot classification\.", text), text
    nprompt = 20 if prompt == "ensemble" else 5
    assert seen["text"].shape[0] == nprompt and seen["audios"].shape[0] == 10 == seen["gold"].shape[0]
    sims = seen["audios"] @ seen["text"].t()
    top2 = sims.topk(2, dim=1)[0]
    assert float((top2[:, 0] - top2[:, 1]).min()) > 1e-6                               # the arg-max is determined
    pred = sims.argmax(1)
    if prompt == "ensemble":
        assert seen["label_map"] == {i: i // 4 for i in range(20)}
        pred = pred // 4                                                               # four prompts per class
    else:
        assert seen["label_map"] == {i: i for i in range(5)}
    precision = (pred == seen["gold"]).sum() / 10 * 100.
    assert f"A->T: p1 = {precision:2.2f} @ 10" in text, text


# ------------------------------------------------------------------ 2. ASMonitor from a toy AudioSet directory
TAG_NAMES = " running.data_name=src_train_toy running.eval_name=src_eval_toy running.test_name=none"


def test_tagging_make_batch_is_the_direct_calls_and_two_steps_run(tag_dir):
    from vipant_amd.data import PcmBatch, TaggingLabels
    from vipant_amd.frontend import KaldiFbank, pcm_wave
    from vipant_amd.monitor import ASMonitor
    root, records, clips = tag_dir
    mon, lines = _monitor("ASMonitor", TAG + " eval=False running.mixup_rate=1.0 running.save_rate=2" + TAG_NAMES, root)
    assert "Total 5 sound classes." in lines and "Instantiate main dataloader from `src_train_toy': total 2 batches." in lines
    assert any(m.startswith("Will do evaluation every") and m.endswith("on 1 batches (src_eval_toy).") for m in lines), lines
    assert mon.testloader is None and mon.gold_file == f"{root}/src_eval_toy.csv" and mon.model.loss_head.soft_targets
    assert [len(row) for row in mon.lid2int] == [6, 6, 8, 6, 6]                         # ragged: one row per class, unpadded
    raw = next(iter(mon.dataloader))
    clips_b, tags = raw[1], raw[3]
    assert isinstance(clips_b, PcmBatch) and isinstance(tags, TaggingLabels) and tags.ids.device.type == "cpu"
    b, p = 4, int((tags.mix_index >= 0).sum())
    assert p >= 2 and clips_b.pcm.shape[0] == b + p and sorted(tags.mix_index[tags.mix_index >= 0].tolist()) == list(range(b, b + p))
    images, audios, text, labels, names = mon.make_batch(raw)
    g = mon._aug_generator()
    fb = KaldiFbank.from_config(mon.cfg.running.audio, float(SR), train=True, device=DEV)
    assert (fb.freq_mask_param, fb.time_mask_param, fb.norms) == (32, 200, (-4.94, 5.76))
    wave, nsamples = pcm_wave(clips_b.pcm.to(DEV), clips_b.nframes, clips_b.channels, mode="first")
    assert wave.shape[0] == b + p
    want = fb(wave, nsamples, masks=fb.draw_masks(b, g), mix=(tags.mix_index, tags.mix_lambda), outputs=b)
    assert audios.shape == (b, 1, T, F) and torch.equal(audios, want)
    full_i = torch.full((b + p,), -1, dtype=torch.int32)
    full_l = torch.ones(b + p)
    full_i[:b], full_l[:b] = tags.mix_index, tags.mix_lambda
    y = ASMonitor.soft_labels(tags.dense().to(DEV), full_i, full_l)[:b]
    assert labels.dtype == torch.float32 and labels.shape == (b, 5) and torch.equal(labels, y)
    assert bool(((labels > 0) & (labels < 1)).any())
    assert text is None and tuple(images.shape) == (b, 1, 1, 1) and names == raw[4]
    mon.learn()
    torch.cuda.synchronize()
    text_out = "\n".join(lines)
    steps = re.findall(r"step (\d)\tlr_w \S+ lr_b \S+ loss (\S+) ", text_out)
    assert [int(s[0]) for s in steps] == [1, 2] and all(math.isfinite(float(s[1])) for s in steps), text_out
    assert re.search(r"mAP = \d+\.\d\d .* @ 4", text_out), text_out                     # the evaluation at step 2 (save_rate) on src_eval_toy


def test_tagging_evaluation_batch_without_mixup(tag_dir):
    from vipant_amd.frontend import KaldiFbank, pcm_wave
    root, records, clips = tag_dir
    mon, lines = _monitor("ASMonitor", TAG + " eval=True running.mixup_rate=0.0" + TAG_NAMES, root)
    assert "Instantiate main dataloader from `src_eval_toy': total 1 batches." in lines and mon.evalloader is None
    assert not mon.model.training and not mon.model.loss_head.soft_targets
    raw = next(iter(mon.dataloader))
    tags = raw[3]
    assert raw[1].pcm.shape[0] == 4 and tags.mix_index.tolist() == [-1] * 4 and raw[4] == [r["id"] for r in records[:4]]
    images, audios, _, labels, names = mon.make_batch(raw)
    fe = KaldiFbank.from_config(mon.cfg.running.audio, float(SR), train=False, device=DEV)
    assert fe.zero_mean_wf
    wave, nsamples = pcm_wave(raw[1].pcm.to(DEV), raw[1].nframes, raw[1].channels, mode="first")
    assert torch.equal(audios, fe(wave, nsamples))                                     # vipant_fbank(zero_mean = 1), no masks
    assert labels.dtype == torch.int64 and torch.equal(labels.cpu(), tags.dense().long())
    assert labels.cpu().tolist()[1] == [0, 1, 0, 1, 0]                                 # t1: classes 1 and 3 (one of them listed twice)
    mon.learn()
    assert re.search(r"mAP = \d+\.\d\d .* @ 4", "\n".join(lines)), lines


def test_tagging_zero_shot_runs_on_the_label_map_s_prompts(tag_dir):
    root, _, _ = tag_dir
    mon, lines = _monitor("ASMonitor", TAG + " eval=True running.zero_shot=True" + TAG_NAMES, root)
    want = [v[2] for v in CF.GOLD["audioset"]["label_maps"][1]["label_map"].values()]
    assert mon.lid2int == want and len({len(row) for row in want}) > 1                  # rows of different lengths: padded per chunk
    mon.learn()
    text = "\n".join(lines)
    assert "(Zero-shot) Evaluating started..." in text and re.search(r"mAP = \d+\.\d\d .* @ 4", text), text


# ------------------------------------------------------------------ 3. without data_root nothing moved
def test_without_data_root_both_trainers_build_their_synthetic_loaders():
    from vipant_amd.monitor import SyntheticFolds, SyntheticTagging
    mon, lines = _monitor("ESCMonitor", ESC + " eval=False")
    assert any("-fold dataloaders from `synthetic'" in m for m in lines) and len(mon.loader_list) == 2
    assert isinstance(mon.loader_list[0][0]()[1], SyntheticFolds._Loader) and isinstance(mon.loader_list[0][1]()[1], SyntheticFolds._Loader)
    batch = next(iter(mon.loader_list[0][0]()[1]))
    assert tuple(batch[0].shape) == (4, T, F) and tuple(mon.make_batch(batch)[0].shape) == (4, 1, T, F)
    mon, lines = _monitor("ASMonitor", TAG + " eval=False")
    assert "Instantiate main dataloader from `synthetic': total 2 batches, 12 sound classes." in lines
    assert isinstance(mon.dataloader, SyntheticTagging) and isinstance(mon.evalloader, SyntheticTagging)
    images, audios, _, labels, _ = mon.make_batch(next(iter(mon.dataloader)))
    assert audios.shape == (4, 1, T, F) and labels.shape == (4, 12)
