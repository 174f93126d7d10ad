"""`running.audio.resample_to=16000` through the trainers on the MI355X, on the toy trees of tests/native_fixture.py (8-bit at 8 kHz,
16-bit at 44.1 kHz, 24-bit at 96 kHz, 32-bit at 48 kHz, float at 192 kHz; geometry and overrides of tests/test_native_trainer_gpu.py).
What a trainer's `make_batch` yields is, bit for bit, the hand composition `pcm_ingest` -> `Resample` -> `KaldiFbank(16000)` with a
generator seeded the same way; with the key at 0 it is the `RateFbank` batch of before.  The 8 kHz clips are 0.8 s long: 12800 samples
at 16 kHz, beyond the crop length of T = 64 frames (11040), so a training batch draws views and masks and an evaluation batch takes
the centred crop -- at the target rate."""
import numpy as np
import pytest
import torch

import clf_fixture as CF
import native_fixture as NF
import test_native_trainer_gpu as NT

pytestmark = pytest.mark.gpu

DEV, T, F = NT.DEV, NT.T, NT.F
TO = " running.audio.resample_to=16000"


def by_hand(mon, clips, train, to, outputs=None, mix=None):
    from vipant_amd.frontend import KaldiFbank, RateFbank, Resample, pcm_ingest, raw_lengths
    n, _ = raw_lengths(clips.nframes, clips.channels, clips.fmt, clips.raw.shape[1])
    wave, ns = pcm_ingest(clips.raw.to(DEV), clips.nframes, clips.channels, clips.fmt, wave_stride=max(8, -(-int(n.max()) // 8) * 8))
    rates = clips.rates
    if to:
        fb, resample = KaldiFbank.from_config(mon.cfg.running.audio, float(to), train=train, device=DEV), Resample(to, device=DEV)
        wave, ns = resample(wave, ns, rates, host_lengths=n)
        n, rates = resample.lengths(n, rates), None
        assert ns.cpu().tolist() == n.tolist() and wave.shape[1] == -(-int(n.max()) // 8) * 8
        assert not any(bool(wave[i, k:].any()) for i, k in enumerate(n.tolist()))
    else:
        fb = RateFbank.from_config(mon.cfg.running.audio, train=train, device=DEV)
    args = (wave, ns) if rates is None else (wave, ns, rates)
    g = mon._aug_generator()
    if mix is not None:
        return fb(*args, masks=fb.draw_masks(outputs, g) if train else None, mix=mix, outputs=outputs)
    assert fb.longer_than_crop(n, rates) and not fb.chain                   # the 0.8 s clip: views when training, the centred crop otherwise
    view = fb.draw_views(len(n), g) if train else True
    return fb(*args, masks=fb.draw_masks(len(n), g) if train else None, view=view)


@pytest.fixture(scope="module")
def us8k_dir(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("us8k_resample"))
    return root, NF.make_us8k_dir(root, seconds=(0.8, 0.25, 0.12, 0.2, 0.08))


@pytest.mark.parametrize("to", [16000, 0])
def test_us8k_make_batch_is_ingest_resample_fbank(us8k_dir, to):
    root, written = us8k_dir
    mon, _ = NT.monitor("ESCMonitor", NT.US8K + NT.ON + f" running.audio.resample_to={to} eval=False", root, extra=["running.prompt=the sound of"])
    raw = next(r for r in mon.loader_list[1][0]()[1] if 8000 in r[0].rates.tolist() and len(set(r[0].rates.tolist())) >= 3)
    NT.check_raw_batch(raw[0], written.values())
    for train in (True, False):                                             # (a held-out fold of the toy tree has one rate: the same batch)
        mon.model.train(train)
        mon.aug_generator = mon._aug_generator()
        audios, _, _ = mon.make_batch(raw)
        assert audios.shape == (raw[0].raw.shape[0], 1, T, F) and bool(torch.isfinite(audios).all())
        assert torch.equal(audios, by_hand(mon, raw[0], train, to))
        if to:                                                              # and it is not the batch the clips' own rates give
            assert not torch.equal(audios, by_hand(mon, raw[0], train, 0))


def test_tagging_partners_are_mixed_at_the_target_rate(tmp_path):
    root = str(tmp_path)
    records = [{"id": f"t{i}", "dir": "bal" if i % 3 == 0 else "", "clip": ["wav"], "frame": "png",
                "labels": [NT.CLASSES[i % 5]] + ([NT.CLASSES[(i + 2) % 5]] if i % 2 else [])} for i in range(8)]
    CF.make_audioset_dir(root, name="src_train_toy", records=records, seconds=(0.05,), channels=(1,))
    CF.make_audioset_dir(root, name="src_eval_toy", records=records[:4], seconds=(0.05,), channels=(1,))
    g = np.random.default_rng(6)
    for i, r in enumerate(records):                                         # the 16-bit clips of the two calls above are replaced
        fmt, rate, ext = NF.SHIPPED[i % 5]
        path = f"{root}/{r['dir'] + '/' if r['dir'] else ''}clip/{r['id']}.wav"
        NF.write_wav(path, NF.codes(g, int(round((0.25, 0.05, 0.12, 0.2, 0.08)[i % 5] * rate)), 1 + i % 2, fmt), fmt, rate, ext)
    mon, _ = NT.monitor("ASMonitor", NT.TAG + NT.ON + TO + " eval=False running.mixup_rate=1.0", root)
    raw = next(iter(mon.dataloader))
    clips, tags = raw[1], raw[3]
    b, mixed = 4, [(i, int(p)) for i, p in enumerate(tags.mix_index.tolist()) if p >= 0]
    assert clips.raw.shape[0] == b + len(mixed) and any(int(clips.rates[i]) != int(clips.rates[p]) for i, p in mixed)
    mon.aug_generator = mon._aug_generator()
    _, audios, _, _, _ = mon.make_batch(raw)
    want = by_hand(mon, clips, True, 16000, outputs=b, mix=(tags.mix_index, tags.mix_lambda))
    assert audios.shape == (b, 1, T, F) and torch.equal(audios, want) and bool(torch.isfinite(audios).all())
