"""The bimodal VA trainer from files (`running.data_root=DIR`): a generated directory in the reference's layout -- 8 clips of 0.4 to
3.1 s (some shorter, some longer than crop_len = 2.61 s), mono and stereo, PNG frames of 37x53 to 96x128 -- goes through the loader,
`pcm_wave`, the log-mel front-end and the image views, and what the worker sees is, bit for bit, the direct calls with a generator
seeded the same way.  Geometry of tests/test_image_view_trainer_gpu.py: 2-block towers, resolution 32, T = 256, F = 64, batch 4,
2 steps.  Without `data_root` the trainer is what it was: the constants below come from the parent commit."""
import hashlib
import json
import re

import numpy as np
import pytest
import torch

import src_fixture as SF
from oracle import fbank_cpu as FB

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
COMMON = ("+model/image=vit_val +model/audio=vit_val +model/text=dummy +optimizer=standard +running/audio=default num_gpus=1 "
          "model.audio.pre_encoder.stride=[16,24] model.image.encoder.layers=2 model.image.resolution=32 running.audio.max_len=256 "
          "running.audio.num_mel_bins=64 running.batch_size=4 running.synthetic_steps=2 optimizer.epochs=1 optimizer.warmup_epoch=1 "
          "running.clip_model_root=/nonexistent")
BIMODAL = "+running=bimodal worker=CVALP monitor=VAMonitor +model/loss=ce model.image.freeze=False " + COMMON
SECONDS = [0.4, 3.1, 1.3, 2.9, 0.9, 2.7, 2.0, 0.6]
CHANNELS = [1, 2, 1, 2, 2, 1, 2, 1]
FRAMES = [(37, 53), (96, 128), (64, 48), (50, 50), (96, 40), (37, 128), (72, 96), (40, 41)]
NAMES = [0, 2, 0, 5, 1, 0, 6, 3]             # frame names per item: 0 = the frame is a string
SR, T, F = 16000, 256, 64
CROP_LEN = int((T / 100 + 0.05) * SR)        # 41760 samples = 2.61 s

# `data_root=""`: the first synthetic batch (sha256 of each slot's bytes) and the loss strings of the two steps, as printed by the
# PARENT commit for BIMODAL + " eval=False" on an MI355X (two runs there gave the same strings): nothing of this pull request may
# move them.
PARENT_SLOTS = [((4, 3, 32, 32), "4971d9a76aa4b8e6e5c2e9b647365bb8bee73fb2fc75e96ebc43b75ffa56da4d"),
                ((4, 256, 64), "f9a1c6647cb6bdcf460637033921c4a22ee76da4eed934c65b630605a9605778"),
                ((4, 1), "66687aadf862bd776c8fc18b8e9f8e20089714856ee233b3902a591d0d5f2925"),
                ((4,), "66687aadf862bd776c8fc18b8e9f8e20089714856ee233b3902a591d0d5f2925")]
PARENT_LOSSES = [("1", "2.787"), ("2", "2.791")]


@pytest.fixture(scope="module")
def src_dir(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("src"))
    records, clips, frames = SF.make_src_dir(root, "src_train_toy", SECONDS, CHANNELS, FRAMES, nframes_per_item=NAMES,
                                             sub_dirs=["", "bal", "", "bal", "", "", "bal", ""])
    with open(f"{root}/src_eval_toy.csv", "w") as f:
        for r in records:
            f.write(json.dumps(r) + "\n")
    assert min(c.shape[0] for c in clips) < CROP_LEN < max(c.shape[0] for c in clips)
    return root, records, clips, frames


def _monitor(ov, tmp=None):
    from vipant_amd import monitor
    from vipant_amd.config import compose
    if tmp is not None:
        ov += f" running.data_root={tmp} running.data_name=src_train_toy running.eval_name=src_eval_toy alias_root={tmp}/out"
    cfg = compose(ov.split())
    cfg.rank = 0
    torch.manual_seed(cfg.seed)
    lines = []
    return monitor.VAMonitor(cfg, lambda m: lines.append(str(m)), DEV), lines


def _losses(lines):
    return re.findall(r"step (\d)\tlr_w \S+ lr_b \S+ loss (\d+\.\d{3})", "\n".join(lines))


def test_two_steps_from_files_and_the_worker_sees_the_direct_calls(src_dir):
    from vipant_amd.data import FrameBatch, PcmBatch
    from vipant_amd.frontend import KaldiFbank, pcm_wave
    from vipant_amd.image_views import ImageViews
    root = src_dir[0]
    mon, lines = _monitor(BIMODAL + " eval=False", root)
    assert "Instantiate main dataloader from `src_train_toy': total 2 (1) batches." in lines
    assert "Will do evaluation every 1000000000.0 steps on 2 batches." in lines
    assert mon.gold_file == f"{root}/src_eval_toy.csv" and mon.evalloader is not None
    raws, seen = [], []
    real_batch, real_forward = mon.make_batch, mon.model.forward

    def spy_batch(batch):
        if mon.model.training:
            raws.append(batch)
        return real_batch(batch)

    def spy_forward(images, audios, text, **kw):
        if mon.model.training:
            seen.append((images, audios))
        return real_forward(images, audios, text, **kw)
    mon.make_batch, mon.model.forward = spy_batch, spy_forward
    mon.learn()
    torch.cuda.synchronize()
    steps = _losses(lines)
    assert [int(s[0]) for s in steps] == [1, 2] and all(np.isfinite(float(s[1])) for s in steps), lines
    assert len(raws) == len(seen) == 2
    # by hand, from a generator seeded the same way and consumed in step order
    g = torch.Generator().manual_seed(int(mon.cfg.seed) + 7 + 1000 * 0)
    fb = KaldiFbank.from_config(mon.cfg.running.audio, float(SR), train=True, device=DEV)
    assert (fb.freq_mask_param, fb.time_mask_param, fb.crop_len, fb.norms, fb.chain) == (32, 200, CROP_LEN, (), {})
    views = 0
    for raw, (images, audios) in zip(raws, seen):
        assert isinstance(raw[0], FrameBatch) and isinstance(raw[1], PcmBatch) and raw[1].pcm.device.type == "cpu"
        clips = raw[1]
        wave, nsamples = pcm_wave(clips.pcm.to(DEV), clips.nframes, clips.channels, mode="first")
        view = fb.draw_views(4, g) if int(clips.nframes.max()) > CROP_LEN else None
        views += view is not None
        want = fb(wave, nsamples, masks=fb.draw_masks(4, g), view=view)
        assert audios.shape == (4, 1, T, F) and audios.dtype == torch.float32
        assert torch.equal(audios, want)
        assert torch.equal(images, ImageViews(32, "clip", device=DEV)(raw[0].frames.to(DEV), hw=raw[0].hw))
        assert images.shape == (4, 3, 32, 32) and bool(torch.isfinite(images).all())
    assert views >= 1                                  # four of the eight clips are longer than crop_len: some batch crops
    # the end-of-epoch evaluation ran on the evaluation index, against it as gold file
    assert any("I->A: P@1" in m and "A->I: t1 = " in m and m.rstrip().endswith("@ 8") for m in lines), lines


def test_the_launch_line_trains_from_a_directory(src_dir, tmp_path):
    import train as entry
    entry.train((BIMODAL + f" eval=False mode=dp verbose=False running.data_root={src_dir[0]} running.data_name=src_train_toy "
                 f"running.eval_name=none alias_root={tmp_path} model_name=t").split())
    torch.cuda.synchronize()
    text = (tmp_path / "t" / "train_0.out").read_text()
    steps = _losses([text])
    assert [int(s[0]) for s in steps] == [1, 2] and all(np.isfinite(float(s[1])) for s in steps), text
    assert "Instantiate main dataloader from `src_train_toy': total 2 (1) batches." in text and "# step 2 # sample 8" in text
    assert "Will do evaluation" not in text                                      # no index of that name: no evaluation loader


def _centre_crop(x, length):
    """RandomCrop.random_crop(train=False) (transform.py:123-141) on a mono fp32 waveform."""
    if x.shape[0] <= length:
        return x
    left = int(round(0.5 * (x.shape[0] - length)))
    old_std = x.std() * 0.5
    cropped = x[left:left + length]
    new_std = cropped.std()
    if new_std < old_std:
        cropped = x[:length]
    out_std = cropped.std()
    if old_std > new_std > out_std:
        cropped = x[-length:]
    return cropped


def _spectrogram64(w):
    """oracle.fbank_cpu.spectrogram_item (no norms, zero-mean waveform) restated in float64."""
    w = w.double()
    w = w - w.mean()
    shift, size, padded = FB.window_properties(SR)
    m = FB.num_frames(w.shape[0], size, shift)
    frames = w.as_strided((m, size), (shift, 1)).clone()
    frames = frames - frames.mean(dim=1, keepdim=True)
    prev = torch.cat([frames[:, :1], frames[:, :-1]], dim=1)
    frames = frames - 0.97 * prev
    frames = frames * torch.hann_window(size, periodic=False, dtype=torch.float64).unsqueeze(0)
    frames = torch.nn.functional.pad(frames, (0, padded - size))
    power = torch.fft.rfft(frames, dim=1).abs().pow(2.0)
    mel = power @ FB.mel_banks(F, padded, SR).double().t()
    x = torch.max(mel, torch.tensor(FB.EPS, dtype=torch.float64)).log()[:T]
    return torch.nn.functional.pad(x, (0, 0, 0, T - x.shape[0]))


def test_evaluation_reads_eval_name_and_its_log_mels_match_the_cpu_oracle(src_dir):
    root, records, clips, _ = src_dir
    mon, lines = _monitor(BIMODAL + " eval=True", root)
    assert "Instantiate main dataloader from `src_eval_toy': total 2 (1) batches." in lines
    assert mon.gold_file == f"{root}/src_eval_toy.csv" and mon.evalloader is None and not mon.model.training
    k = 0
    for raw in mon.dataloader:                                              # sequential: the index order
        got = mon.make_batch(raw)[1].cpu()
        assert list(raw[4]) == [r["id"] for r in records[k:k + 4]]
        for i in range(4):
            w = _centre_crop(torch.from_numpy(clips[k + i][:, 0].copy()).float() / 32768, CROP_LEN)
            ref = FB.spectrogram_item(w, SR, T, F, norms=(), zero_mean_wf=True)
            own = (ref - _spectrogram64(w).float()).abs()
            err = (got[i, 0] - ref).abs()
            print(f"clip {k + i} ({clips[k + i].shape}): max {float(err.max()):.3e} mean {float(err.mean()):.3e}; oracle's own distance "
                  f"max {float(own.max()):.3e} mean {float(own.mean()):.3e}")
            assert err.max() < 2e-3 + float(own.max()), (k + i, float(err.max()))
            assert err.mean() < 5e-5 + float(own.mean()), (k + i, float(err.mean()))
        k += 4
    assert k == 8
    mon.learn()
    torch.cuda.synchronize()
    assert "Evaluating started..." in lines and not _losses(lines)
    report = lines[-1]
    assert "I->A: P@1" in report and "A->I: P@1" in report and "I->A: t1 = " in report and report.rstrip().endswith("@ 8"), lines


def test_eval_norms_prints_the_statistics_and_does_not_train(src_dir, monkeypatch):
    from vipant_amd import monitor
    root = src_dir[0]
    mels = []
    real = monitor.VAMonitor.make_batch

    def spy(self, batch):
        out = real(self, batch)
        mels.append(out[1].detach().cpu().double().numpy())
        return out
    monkeypatch.setattr(monitor.VAMonitor, "make_batch", spy)
    mon, lines = _monitor(BIMODAL + " eval=False running.audio.eval_norms=True running.audio.norms=[-4.94,5.76]", root)
    mon.learn()
    assert mon.model is None and not _losses(lines) and "Training started..." not in lines
    x = np.concatenate(mels)[:, 0]
    assert x.shape == (8, T, F)
    mean = x.mean(axis=(1, 2)).mean()
    std = np.sqrt((x ** 2).mean(axis=(1, 2)).mean() - mean ** 2)
    said = [m for m in lines if m.startswith("MEAN: ")]
    assert len(said) == 1 and lines[-1] == said[0], lines
    got = re.fullmatch(r"MEAN: \[(\S+)\] STD: \[(\S+)\]", said[0])
    assert got is not None, said
    print(said[0], mean, std)
    assert abs(float(got.group(1)) - mean) <= 1e-5 * abs(mean) and abs(float(got.group(2)) - std) <= 1e-5 * std
    # raw log-mels: `norms` is off under the key, whatever the config says -- the padding behind the five clips of at most 2 s is 0
    assert sum(bool(np.all(x[c, 200:] == 0.0)) for c in range(8)) == 5 and std > 1.0


def test_without_data_root_the_trainer_is_the_parent_s():
    mon, lines = _monitor(BIMODAL + " eval=False")
    assert "Instantiate main dataloader from `synthetic': total 2 batches." in lines
    raw = next(iter(mon.dataloader))
    for t, (shape, digest) in zip(raw[:4], PARENT_SLOTS):
        assert tuple(t.shape) == shape and hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest() == digest
    assert raw[4] == [f"synthetic-0-0-{i}" for i in range(4)]
    mon.learn()
    torch.cuda.synchronize()
    assert _losses(lines) == PARENT_LOSSES, lines
