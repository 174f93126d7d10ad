"""The AT trainer from files (`monitor=VALMonitor running.data_root=DIR`): generated AudioCaps and Clotho directories in the reference's
layout go through the caption datasets, the tokenizer, `pcm_wave`, the log-mel front-end and the towers.  What the worker sees is, bit
for bit, the direct front-end calls with a generator seeded the same way; text batches are as wide as their longest caption; an
evaluation batch holds 5 b text rows against b clips and its report is the reference's, restated here; Clotho runs at 44.1 kHz (padded
window 2048).  The model is the shrunk AT layout of tests/test_model_gpu.py `test_at_step_with_frozen_text_tower`: 2 blocks per tower,
T = 256, F = 64, no image, batch 4.  Without `data_root` the trainer is what it was: the constants below come from the parent commit."""
import hashlib
import re

import numpy as np
import pytest
import torch

import at_fixture as AF
from oracle import fbank_cpu as FB

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
AT = ("+running=trimodal monitor=VALMonitor worker=CVALP mode=dp num_gpus=1 +model/image=vit_val +model/audio=vit_val "
      "+model/text=transformer_val +model/loss=ce_val +optimizer=standard +running/audio=default "
      "model.audio.pre_encoder.stride=[16,24] running.siamese.alive=True running.imagine=False model.loss.va=False "
      "model.image.encoder.layers=2 model.text.encoder.layers=2 model.image.resolution=32 running.audio.max_len=256 "
      "running.audio.num_mel_bins=64 running.batch_size=4 running.synthetic_steps=2 running.epochs=1 optimizer.warmup_epoch=1 "
      "running.clip_model_root=/nonexistent")
SECONDS = [0.4, 3.1, 1.3, 2.9, 0.9, 2.7, 2.0, 0.6]
CHANNELS = [1, 2, 1, 2, 2, 1, 2, 1]
FRAMES = [(37, 53), (96, 128), (64, 48), (50, 50), (96, 40), (37, 128), (72, 96), (40, 41)]
SR, T, F = 16000, 256, 64
CROP_LEN = int((T / 100 + 0.05) * SR)        # 41760 samples = 2.61 s
# The seed of the generated clips and frames.  The evaluation test compares a report that depends on the ORDER of similarities, and
# refuses to judge when two similarities of a row lie within 1e-6 of each other.  With 8 x 39 + 40 x 7 neighbouring pairs at a typical
# distance of 2e-3 (untrained towers) that happens for about one seed in seven, and it did for the first seed tried (5: 1.4e-7).  Of
# the seeds 11 .. 17, measured on an MI355X, none has such a pair; 11 has the widest margin (smallest distances 1.68e-5 clip x caption,
# 4.11e-5 caption x clip, the same figures in a second run).  The 1e-6 rule and the comparison are as they were.
CLIP_SEED = 11
CLOTHO_SECONDS, CLOTHO_SR, CLOTHO_T = [0.5, 1.5, 0.8, 1.1], 44100, 128
CLOTHO_CROP = int((CLOTHO_T / 100 + 0.05) * CLOTHO_SR)       # 58653 samples = 1.33 s

# `data_root=""`: the first synthetic batch (shape and sha256 of each slot's bytes) and the loss strings of the two steps, as printed
# by the PARENT commit for AT + " eval=False" on an MI355X (two runs there gave the same strings): nothing of this pull request may
# move them.
PARENT_SLOTS = [((4, 1, 1, 1), "374708fff7719dd5979ec875d56cd2286f6d3cf7ec317a3b25632aab28ec37bb"),
                ((4, 256, 64), "f9a1c6647cb6bdcf460637033921c4a22ee76da4eed934c65b630605a9605778"),
                ((4, 60), "1d6f2f3a3b75b56e4ba4fda1014d452f54b95032c07d8e401226a4c580c21f69"),
                ((4,), "66687aadf862bd776c8fc18b8e9f8e20089714856ee233b3902a591d0d5f2925")]
PARENT_LOSSES = [("1", "2.914", "al 2.914"), ("2", "2.848", "al 2.848")]


@pytest.fixture(scope="module")
def at_dir(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("at"))
    records, clips, frames = AF.make_audiocaps_dir(root, "audiocaps_train_toy", SECONDS, CHANNELS, frame_hw=FRAMES,
                                                   sub_dirs=["", "bal", "", "bal", "", "", "bal", ""], seed=CLIP_SEED)
    AF.write_index(root, "audiocaps_eval_toy", records)
    AF.write_index(root, "audiocaps_four_toy", records[:4])
    assert min(c.shape[0] for c in clips) < CROP_LEN < max(c.shape[0] for c in clips)
    from vipant_amd.tokenizer import load_tokenizer, tokenize
    tok = load_tokenizer(AF.BPE)
    bpe = {r["id"]: tokenize(r["captions"], as_list=True, tokenizer=tok) for r in records}
    lengths = sorted(len(row) for rows in bpe.values() for row in rows)
    assert lengths[0] == 6 and lengths[-1] == 40 and all(len(rows) == 5 for rows in bpe.values())
    assert len({tuple(row) for rows in bpe.values() for row in rows}) == 40          # no two captions alike: no two text features alike
    return root, records, clips, frames, bpe


@pytest.fixture(scope="module")
def clotho_dir(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("clotho"))
    rows, clips = AF.make_clotho_dir(root, "development", CLOTHO_SECONDS, rate=CLOTHO_SR)
    AF.make_clotho_dir(root, "validation", [0.5], rate=16000)                   # a file at another rate
    assert min(c.shape[0] for c in clips) < CLOTHO_CROP < max(c.shape[0] for c in clips)
    return root, rows, clips


def _monitor(ov, root=None, names="running.data_name=audiocaps_train_toy running.eval_name=audiocaps_eval_toy", extra=()):
    from vipant_amd import monitor
    from vipant_amd.config import compose
    if root is not None:
        ov += f" running.data_root={root} running.bpe_path={AF.BPE} alias_root={root}/out {names}"
    cfg = compose(ov.split() + list(extra))                 # `extra`: overrides whose value holds blanks
    cfg.rank = 0
    torch.manual_seed(cfg.seed)
    lines = []
    return monitor.VALMonitor(cfg, lambda m: lines.append(str(m)), DEV), lines


def _losses(lines):
    return re.findall(r"step (\d)\tlr_w \S+ lr_b \S+ loss (\d+\.\d{3}) (.*?) \S+ samples/s", "\n".join(lines))


def _spy(mon, raws, seen, training=True):
    real_batch, real_forward = mon.make_batch, mon.model.forward

    def spy_batch(batch):
        if mon.model.training == training:
            raws.append(batch)
        return real_batch(batch)

    def spy_forward(images, audios, text, **kw):
        if mon.model.training == training:
            seen.append((images, audios, text))
        return real_forward(images, audios, text, **kw)
    mon.make_batch, mon.model.forward = spy_batch, spy_forward


# ------------------------------------------------------------------ 1. training
def test_two_steps_from_an_audiocaps_index_and_the_worker_sees_the_direct_calls(at_dir):
    from vipant_amd.data import PcmBatch
    from vipant_amd.frontend import KaldiFbank, pcm_wave
    root, records, _, _, bpe = at_dir
    mon, lines = _monitor(AT + " eval=False", root, names="running.data_name=audiocaps_train_toy running.eval_name=audiocaps_eval_toy "
                                                          "running.test_name=audiocaps_four_toy")
    assert "Instantiate main dataloader from `audiocaps_train_toy': total 2 batches." in lines
    assert "Will do evaluation every 1000000000.0 steps on 2 batches (audiocaps_eval_toy)." in lines
    assert "Will do test every 1000000000.0 steps on 1 batches (audiocaps_four_toy)." in lines
    assert mon.gold_file == f"{root}/audiocaps_eval_toy.csv" and mon.gold_file_test == f"{root}/audiocaps_four_toy.csv"
    assert mon.evalloader is not None and mon.testloader is not None
    assert mon.model.image_head is None and mon.model.text_head is not None
    raws, seen = [], []
    _spy(mon, raws, seen)
    before = {k: v.detach().clone() for k, v in mon.model.named_parameters()}
    mon.learn()
    torch.cuda.synchronize()
    steps = _losses(lines)
    assert [int(s[0]) for s in steps] == [1, 2] and all(np.isfinite(float(s[1])) and s[2].startswith("al ") for s in steps), lines
    assert len(raws) == len(seen) == 2
    # by hand, from a generator seeded the same way and consumed in step order
    g = torch.Generator().manual_seed(int(mon.cfg.seed) + 7 + 1000 * 0)
    fb = KaldiFbank.from_config(mon.cfg.running.audio, float(SR), train=True, device=DEV)
    assert (fb.freq_mask_param, fb.time_mask_param, fb.crop_len, fb.norms, fb.chain) == (32, 200, CROP_LEN, (), {})
    views, names = 0, []
    for raw, (images, audios, text) in zip(raws, seen):
        assert isinstance(raw[1], PcmBatch) and raw[1].pcm.device.type == "cpu"
        clips = raw[1]
        wave, nsamples = pcm_wave(clips.pcm.to(DEV), clips.nframes, clips.channels, mode="first")
        view = fb.draw_views(4, g) if int(clips.nframes.max()) > CROP_LEN else None
        views += view is not None
        want = fb(wave, nsamples, masks=fb.draw_masks(4, g), view=view)
        assert audios.shape == (4, 1, T, F) and audios.dtype == torch.float32
        assert torch.equal(audios, want)
        # the dummy image slot passes through untouched
        assert tuple(raw[0].shape) == (4, 1, 1, 1) and tuple(images.shape) == (4, 1, 1, 1) and images.is_cuda
        assert torch.equal(images.cpu(), raw[0])
        # text: as wide as the batch's longest caption, every row one of its clip's captions and zeros behind it
        rows = text.cpu().tolist()
        assert text.dtype == torch.int64 and text.is_cuda and torch.equal(text.cpu(), raw[2]) and len(rows) == 4
        lens = [row.index(49407) + 1 for row in rows]
        print(f"training batch {raw[4]}: caption lengths {lens}, width {text.shape[1]}")
        assert text.shape[1] == max(lens) < 77
        for name, row, n in zip(raw[4], rows, lens):
            assert row[:n] in bpe[name] and not any(row[n:]), (name, row)
        names += list(raw[4])
    assert sorted(names) == sorted(r["id"] for r in records)
    assert views >= 1                                  # four of the eight clips are longer than crop_len: some batch crops
    moved = {k for k, v in mon.model.named_parameters() if not torch.equal(v.detach(), before[k])}
    assert all(k.startswith(("audio_head.", "loss_head.")) for k in moved) and len(moved) > 30, sorted(moved)[:8]
    # the end-of-epoch evaluation ran on the evaluation index, then on the test index
    reports = [m for m in lines if "A->T: t1 = " in m]
    assert len(reports) == 2 and "@ 8\nREFERENCE" in reports[0] and "@ 4\nREFERENCE" in reports[1], lines


# ------------------------------------------------------------------ 2. evaluation: 5 b captions against b clips
def _reference_report(x1s, x2s):
    """cvap/module/decoder/loss_head.py:135-168 (the 1 v 5 branch of `report`) and :68-107 (`retrieval_metrics`, `retrieval_eval`)
    restated: x1s [n, E] clips, x2s [5 n, E] captions, float32 on the CPU."""
    def metrics(ranks, msg):
        nsample = ranks.shape[0]
        r = [torch.where(ranks < k)[0].shape[0] / nsample * 100. for k in (1, 5, 10, 50)]
        med, avg = ranks.median() + 1, ranks.mean() + 1
        return f"{msg}: R@1 {r[0]:2.2f} R5 {r[1]:2.2f} R10 {r[2]:2.2f} R50 {r[3]:2.2f} MED {med:2.2f} AVG {avg:2.2f}"
    n, k = x1s.shape[0], 5
    x12, x21 = x1s @ x2s.t(), x2s @ x1s.t()
    ind_12, ind_21 = x12.argsort(descending=True), x21.argsort(descending=True)
    labels = torch.arange(n * k).unsqueeze(-1)
    r12 = torch.where(ind_12.repeat_interleave(5, dim=0) == labels)[1].reshape(-1, 5)
    t1 = (r12 < 1).sum(-1).sum() / (1 * r12.shape[0]) * 100.
    t5 = (r12 < 5).sum(-1).sum() / (5 * r12.shape[0]) * 100.
    mean = r12.min(-1)[0].float().mean() + 1
    p_12 = f"A->T: t1 = {t1:2.2f} t5 = {t5:2.2f} mR = {mean:2.2f}"
    labels = torch.arange(n).unsqueeze(-1).repeat(1, 5).view(-1, 1)
    r21 = torch.where(ind_21 == labels)[1]
    t1 = torch.where(r21 < 1)[0].shape[0] / r21.shape[0] * 100.
    t5 = torch.where(r21 < 5)[0].shape[0] / r21.shape[0] * 100.
    mean = r21.float().mean() + 1
    p_21 = f"T->A: t1 = {t1:2.2f} t5 = {t5:2.2f} mR = {mean:2.2f}"
    ranks = torch.zeros(n)
    for i in range(n):
        rank = 1e9
        for j in range(i * k, i * k + k):
            rank_j = torch.where(ind_12[i:i + 1] == j)[1][0]
            if rank_j < rank:
                rank = rank_j
        ranks[i] = rank
    msg_12 = metrics(ranks, "A->T")
    ranks = torch.zeros(n * k)
    for i in range(n):
        for j in range(k):
            ranks[i * k + j] = torch.where(ind_21[i * k + j:i * k + j + 1] == i)[1][0]
    msg_21 = metrics(ranks, "T->A")
    return f"{p_12} {p_21} @ {n}\nREFERENCE\n{msg_12}\n{msg_21}", (x12, x21)


def test_evaluation_scores_five_captions_per_clip_and_reports_as_the_reference(at_dir):
    root, records, _, _, bpe = at_dir
    mon, lines = _monitor(AT + " eval=True", root)
    assert "Instantiate main dataloader from `audiocaps_eval_toy': total 2 batches." in lines
    assert mon.gold_file == f"{root}/audiocaps_eval_toy.csv" and mon.evalloader is None and not mon.model.training
    raws, seen, fed = [], [], []
    _spy(mon, raws, seen, training=False)
    head = mon.model.loss_head
    real_infer = head.infer

    def spy_infer(x1, x2, x3, *args, **kwargs):
        fed.append((x1, x2.detach().float().cpu(), x3.detach().float().cpu(), kwargs.get("normalized", False), list(kwargs["names"])))
        return real_infer(x1, x2, x3, *args, **kwargs)
    head.infer = spy_infer
    mon.learn()
    torch.cuda.synchronize()
    assert "Evaluating started..." in lines and "# sample 8;" in "\n".join(lines), lines
    assert len(fed) == 2 and [tuple(raw[2].shape) for raw in raws] == [(20, 40), (20, 35)]       # the width follows the batch
    k = 0
    for raw, (images, audios, text), (x1, x2, x3, normalized, names) in zip(raws, seen, fed):
        E = x2.shape[1]
        assert x1 is None and x2.shape == (4, E) and x3.shape == (20, E) and E == 512
        assert names == list(raw[4]) == [r["id"] for r in records[k:k + 4]] and tuple(images.shape) == (4, 1, 1, 1)
        rows = text.cpu().tolist()
        want = [row for r in records[k:k + 4] for row in bpe[r["id"]]]            # a clip's captions contiguous, in clip order
        assert text.dtype == torch.int64 and len(rows) == 20
        assert all(row[:len(w)] == w and not any(row[len(w):]) for row, w in zip(rows, want))
        k += 4
    assert sum(len(f[4]) for f in fed) == 8
    norm = lambda x, done: x if done else x / x.norm(dim=-1, keepdim=True)
    x1s = torch.cat([norm(f[1], f[3]) for f in fed])
    x2s = torch.cat([norm(f[2], f[3]) for f in fed])
    want, sims = _reference_report(x1s, x2s)
    for name, sim in zip(("clip x caption", "caption x clip"), sims):
        gaps = sim.sort(dim=1)[0].diff(dim=1)
        print(f"{name}: smallest distance of two similarities of a row {float(gaps.min()):.3e}")
        assert float(gaps.min()) > 1e-6, (f"{name}: two similarities of a row lie within 1e-6 of each other ({float(gaps.min()):.3e}); "
                                          "their order, and with it the report, is not determined")
    report = lines[-1]
    print(report)
    assert "A->T: t1 = " in report and "T->A: t1 = " in report and "@ 8\nREFERENCE\n" in report
    assert report == "\nAL: " + want


# ------------------------------------------------------------------ 3. Clotho at 44.1 kHz
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


def _spectrogram64(w, rate, max_len, bins):
    """oracle.fbank_cpu.spectrogram_item (no norms, zero-mean waveform) restated in float64."""
    w = w.double()
    w = w - w.mean()
    shift, size, padded = FB.window_properties(rate)
    m = FB.num_frames(w.shape[0], size, shift)
    frames = w.as_strided((m, size), (shift, 1)).clone()
    frames = frames - frames.mean(dim=1, keepdim=True)
    prev = torch.cat([frames[:, :1], frames[:, :-1]], dim=1)
    frames = frames - 0.97 * prev
    frames = frames * torch.hann_window(size, periodic=False, dtype=torch.float64).unsqueeze(0)
    frames = torch.nn.functional.pad(frames, (0, padded - size))
    power = torch.fft.rfft(frames, dim=1).abs().pow(2.0)
    mel = power @ FB.mel_banks(bins, padded, rate).double().t()
    x = torch.max(mel, torch.tensor(FB.EPS, dtype=torch.float64)).log()[:max_len]
    return torch.nn.functional.pad(x, (0, 0, 0, max_len - x.shape[0]))


def test_clotho_at_44100_hz(clotho_dir):
    from vipant_amd.data import build_audio_text_dataloader
    from vipant_amd.errors import VipantError
    from vipant_amd.frontend import pcm_wave
    from vipant_amd.tokenizer import tokenize
    root, rows, clips = clotho_dir
    mon, lines = _monitor(AT + f" eval=True running.sample_rate=44100 running.audio.max_len={CLOTHO_T}", root,
                          names="running.eval_name=clotho_development", extra=["running.prompt=the sound of"])
    assert "Instantiate main dataloader from `clotho_development': total 1 batches." in lines
    prompt = tokenize("the sound of", as_list=True)[0][1:4]
    assert prompt == [518, 3608, 539]
    raw = next(iter(mon.dataloader))
    images, audios, text, _, names = mon.make_batch(raw)
    fb = mon.pcm_frontend(False, CLOTHO_SR)
    assert (fb.size, fb.shift, fb.padded, fb.crop_len) == (1102, 441, 2048, CLOTHO_CROP)
    assert raw[1].sample_rate == CLOTHO_SR and names == [r["file_name"] for r in rows]
    wave, nsamples = pcm_wave(raw[1].pcm.to(DEV), raw[1].nframes, raw[1].channels, mode="first")
    assert int(raw[1].nframes.max()) > CLOTHO_CROP
    assert audios.shape == (4, 1, CLOTHO_T, F) and torch.equal(audios, fb(wave, nsamples, masks=None, view=True))
    got = audios.cpu()
    for i in range(4):
        w = _centre_crop(torch.from_numpy(clips[i][:, 0].copy()).float() / 32768, CLOTHO_CROP)
        ref = FB.kaldi_fbank(w - w.mean(), 44100., F)[:CLOTHO_T]                    # zero-mean waveform, no norms
        assert ref.shape[0] == min(CLOTHO_T, FB.num_frames(w.shape[0], 1102, 441))
        ref = torch.nn.functional.pad(ref, (0, 0, 0, CLOTHO_T - ref.shape[0]))
        own = (ref - _spectrogram64(w, float(CLOTHO_SR), CLOTHO_T, F).float()).abs()
        err = (got[i, 0] - ref).abs()
        print(f"clip {i} ({clips[i].shape}): max {float(err.max()):.3e} mean {float(err.mean()):.3e}; oracle's own distance "
              f"max {float(own.max()):.3e} mean {float(own.mean()):.3e}")
        assert err.max() < 2e-3 + float(own.max()), (i, float(err.max()))
    rows_ = text.cpu().tolist()
    assert text.shape[0] == 20 and text.shape[1] < 77 and all(row[0] == 49406 and row[1:4] == prompt for row in rows_)
    mon.learn()
    torch.cuda.synchronize()
    assert "A->T: t1 = " in lines[-1] and "@ 4\nREFERENCE" in lines[-1], lines
    # a file at another rate in this run
    _, other = build_audio_text_dataloader(mon.cfg, "clotho_validation", shuffle=False, train=False)
    with pytest.raises(VipantError, match=r"validation/clip 00 - take\.wav: sample rate 16000 Hz, but running\.sample_rate = 44100"):
        next(iter(other))


# ------------------------------------------------------------------ 4. the launch line
def test_the_launch_line_trains_from_a_directory(at_dir, tmp_path):
    import train as entry
    common = (f"alias_root={tmp_path} model_name=t port=1 num_gpus=1 mode=dp num_proc=2 eval=False verbose=False "
              "+model/image=vit_val +model/audio=vit_val +optimizer=standard +running/audio=default "
              "model.audio.pre_encoder.in_channels=3 model.audio.pre_encoder.stride=[16,24] optimizer.warmup=False "
              "running.audio.norms=[-4.93839311,5.75751113] model.image.encoder.layers=1 running.audio.max_len=256 "
              "running.audio.num_mel_bins=64 running.synthetic_steps=2 running.epochs=1 running.peep_rate=1").split()
    at = ["+running=trimodal", "monitor=VALMonitor", "worker=CVALP", "+model/text=transformer_val", "+model/loss=ce_val",
          "running.siamese.alive=True", "running.imagine=False", "model.loss.va=False", "running.batch_size=4",
          "model.text.encoder.layers=1", "model_file=notafile", "+running.rnd_cap=True"] + common
    entry.train(at + [f"running.data_root={at_dir[0]}", "running.data_name=audiocaps_train_toy", "running.eval_name=audiocaps_eval_toy",
                      f"running.bpe_path={AF.BPE}", "running.clip_model_root=/nonexistent"])
    torch.cuda.synchronize()
    text = (tmp_path / "t" / "train_0.out").read_text()
    steps = _losses([text])
    assert [int(s[0]) for s in steps] == [1, 2] and all(np.isfinite(float(s[1])) for s in steps), text
    assert "Instantiate main dataloader from `audiocaps_train_toy'" in text and "# step 2 # sample 8" in text
    assert "Will do evaluation every" in text and "(audiocaps_eval_toy)." in text
    assert "# sample 8;" in text and "A->T: t1 = " in text and "@ 8\nREFERENCE" in text       # the end-of-epoch evaluation
    ck = torch.load(tmp_path / "t" / "00000002.pth", weights_only=False)
    assert len(ck["model"]) == 4 and "encoder.resblocks.0.attn.in_proj_weight" in ck["model"][1]
    assert "loss_head_al.logit_scale" in ck["model"][3] and ck["cfg"]["worker"] == "CVALP"
    assert ck["cfg"]["running"]["data_name"] == "audiocaps_train_toy"


# ------------------------------------------------------------------ 5. imagine: frames beside clips and captions
def test_imagine_sends_frames_through_the_image_views(at_dir):
    from vipant_amd.data import FrameBatch
    from vipant_amd.image_views import ImageViews
    root = at_dir[0]
    ov = AT.replace("running.imagine=False model.loss.va=False", "running.imagine=True model.loss.va=True")
    mon, lines = _monitor(ov + " eval=False running.save_epoch=False", root,
                          names="running.data_name=audiocaps_four_toy running.eval_name=none")
    assert mon.model.image_head is not None and mon.evalloader is None
    assert "Instantiate main dataloader from `audiocaps_four_toy': total 1 batches." in lines
    raws, seen = [], []
    _spy(mon, raws, seen)
    mon.learn()
    torch.cuda.synchronize()
    assert len(raws) == len(seen) == 1
    raw, (images, audios, text) = raws[0], seen[0]
    assert isinstance(raw[0], FrameBatch) and raw[0].frames.dtype == torch.uint8 and raw[0].frames.device.type == "cpu"
    assert sorted(raw[0].hw.tolist()) == sorted([list(hw) for hw in FRAMES[:4]])
    assert images.shape == (4, 3, 32, 32) and torch.equal(images, ImageViews(32, "clip", device=DEV)(raw[0].frames.to(DEV), hw=raw[0].hw))
    assert audios.shape == (4, 1, T, F) and text.shape[0] == 4 and text.shape[1] < 77
    steps = _losses(lines)
    assert len(steps) == 1 and np.isfinite(float(steps[0][1])), lines
    assert re.fullmatch(r"va \d+\.\d{3} al \d+\.\d{3}", steps[0][2]), steps


# ------------------------------------------------------------------ 6. statistics run
def test_eval_norms_prints_the_statistics_and_does_not_train(at_dir):
    mon, lines = _monitor(AT + " eval=False running.audio.eval_norms=True running.audio.norms=[-4.94,5.76]", at_dir[0])
    mon.learn()
    assert mon.model is None and not _losses(lines) and "Training started..." not in lines
    said = [m for m in lines if m.startswith("MEAN: ")]
    assert len(said) == 1 and lines[-1] == said[0] and re.fullmatch(r"MEAN: \[(\S+)\] STD: \[(\S+)\]", said[0]), lines
    assert len([m for m in lines if re.fullmatch(r"step \d", m)]) == 2


# ------------------------------------------------------------------ 7. what did not move, and what is still refused
def test_without_data_root_the_trainer_is_the_parent_s():
    mon, lines = _monitor(AT + " eval=False")
    assert "Instantiate main dataloader from `synthetic': total 2 batches." in lines
    raw = next(iter(mon.dataloader))
    for t, (shape, digest) in zip(raw[:4], PARENT_SLOTS):
        assert tuple(t.shape) == shape and hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest() == digest
    assert raw[4] == [f"synthetic-0-0-{i}" for i in range(4)]
    mon.learn()
    torch.cuda.synchronize()
    assert _losses(lines) == PARENT_LOSSES, lines


def test_the_audioset_names_are_still_refused(at_dir):
    from vipant_amd.errors import VipantError
    for name in ("src_train_toy", "npz_train_toy"):
        with pytest.raises(VipantError, match="`audiocaps` or `clotho`"):
            _monitor(AT + " eval=False", at_dir[0], names=f"running.data_name={name}")
    with pytest.raises(ValueError, match=r"^unrecognized dataset `esc50`\.$"):
        _monitor(AT + " eval=False", at_dir[0], names="running.data_name=esc50")
    with pytest.raises(VipantError, match=r"running\.bpe_path"):
        _monitor(AT + f" eval=False running.data_root={at_dir[0]} running.data_name=audiocaps_train_toy")
