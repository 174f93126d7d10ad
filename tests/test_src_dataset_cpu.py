"""The raw-file image-audio dataset on the host (vipant_amd/data): index, path and frame-choice rules against what the reference's own
`_process_item` recorded (tests/golden/src_dataset.json, made by tests/golden/make_golden_src_dataset.py), the decoders, the fallback
rules, the collator's containers, worker independence -- and the refusals of `vipant_pcm_wave`, which need no device."""
import json
import math
import os
import sys
import warnings

import numpy as np
import pytest
import torch

import src_fixture as SF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "src_dataset.json")))


def _rcfg(root, **kw):
    from vipant_amd.config import to_config
    base = dict(data_root=str(root), eval_samples=5184, train_samples=1.0, frame_key="frame", frame_emb=None, resolution=32, embed_dim=16,
                sample_rate=16000, batch_size=4)
    base.update(kw)
    return to_config(base)


def _index(root, name, records):
    with open(f"{root}/{name}.csv", "w") as f:
        for r in records:
            f.write(json.dumps(r) + "\n")


# ------------------------------------------------------------------ 1. index rules against the reference's record
@pytest.mark.parametrize("case", range(len(GOLD["cases"])))
def test_paths_and_evaluation_frames_are_the_reference_s(tmp_path, case):
    from vipant_amd.data import ImageAudioSrc
    c = GOLD["cases"][case]
    records = [{(c["clip_key"] if k == "clip" else k): v for k, v in r.items()} for r in GOLD["records"]]
    assert len(records) == 7 and [len(r["frame"]) for r in records if not isinstance(r["frame"], str)] == [1, 2, 5, 6, 2]
    _index(tmp_path, "src_toy", records)
    ds = ImageAudioSrc(_rcfg(tmp_path, frame_emb=c["frame_emb"]), "src_toy", train=False)
    assert ds.aclip_key == c["clip_key"] and len(ds) == 7
    for i, want in enumerate(c["items"]):
        got = ds._process_item(i)
        rebased = [None if v is None else v.replace("ROOT", str(tmp_path), 1)
                   for v in (want["name"], want["clip_file"], want["frame_file"], want["frame_emb_file"])]
        rebased[0] = want["name"]
        assert list(got) == rebased, (i, got, rebased)
    picked = [it["frame_index"] for it in c["items"] if it["frame_index"] is not None]
    assert picked[:4] == [0, 0, 2, 2] == [int(math.ceil(n / 2)) - 1 for n in (1, 2, 5, 6)]


def test_a_record_without_dir_reads_from_the_root(tmp_path):
    from vipant_amd.data import ImageAudioSrc
    _index(tmp_path, "src_toy", [{"id": "x", "clip": ["wav"], "frame": "png"}, {"id": "y", "dir": "d", "clip": ["wav"], "frame": "png"}])
    ds = ImageAudioSrc(_rcfg(tmp_path), "src_toy", train=False)
    assert ds._process_item(0)[1:3] == (f"{tmp_path}/clip/x.wav", f"{tmp_path}/frame/x.png")
    assert ds._process_item(1)[1:3] == (f"{tmp_path}/d/clip/y.wav", f"{tmp_path}/d/frame/y.png")


def test_truncation_fraction_and_missing_index(tmp_path):
    from vipant_amd._ffi import VipantError
    from vipant_amd.data import ImageAudioSrc, build_image_audio_dataloader
    records = [{"id": f"r{i}", "dir": "", "clip": ["wav"], "frame": "png"} for i in range(20)]
    _index(tmp_path, "src_toy", records)
    assert len(ImageAudioSrc(_rcfg(tmp_path, eval_samples=5), "src_toy", train=False)) == 5
    assert len(ImageAudioSrc(_rcfg(tmp_path, eval_samples=5), "src_toy", train=True)) == 20          # training reads every line
    part = ImageAudioSrc(_rcfg(tmp_path, train_samples=0.25), "src_toy", train=True, seed=4)
    same = ImageAudioSrc(_rcfg(tmp_path, train_samples=0.25), "src_toy", train=True, seed=4)
    other = ImageAudioSrc(_rcfg(tmp_path, train_samples=0.25), "src_toy", train=True, seed=5)
    ids = [r["id"] for r in part.dataset]
    assert len(ids) == 5 == len(set(ids)) and ids == [r["id"] for r in same.dataset] and ids != [r["id"] for r in other.dataset]
    assert ids != [f"r{i}" for i in range(5)]                                                        # a permutation, not the head
    assert len(ImageAudioSrc(_rcfg(tmp_path, train_samples=0.25), "src_toy", train=False)) == 20     # the fraction is a training rule
    with pytest.raises(VipantError, match=r"src_none\.csv is not a file\."):
        ImageAudioSrc(_rcfg(tmp_path), "src_none", train=True)
    from vipant_amd.config import to_config
    cfg = to_config({"seed": 1, "num_proc": 0, "running": dict(_rcfg(tmp_path))})
    with pytest.raises(VipantError, match="npz datasets: not built"):
        build_image_audio_dataloader(cfg, "npz_toy", False, False)
    with pytest.raises(VipantError, match="unrecognized dataset `toy`"):
        build_image_audio_dataloader(cfg, "toy", False, False)


# ------------------------------------------------------------------ 2. decoders
@pytest.mark.parametrize("ch", [1, 2, 6])
def test_read_wav_equals_scipy(tmp_path, ch):
    from scipy.io import wavfile
    from vipant_amd.data import read_wav
    g = np.random.default_rng(ch)
    pcm = g.integers(-32768, 32768, size=(1001, ch), dtype=np.int64).astype(np.int16)
    pcm[0, :], pcm[1, :] = -32768, 32767
    path = f"{tmp_path}/c{ch}.wav"
    SF.write_wav(path, pcm, rate=22050 if ch == 6 else 16000)
    got, rate = read_wav(path)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want_rate, want = wavfile.read(path)
    assert rate == want_rate and got.dtype == np.int16 and got.shape == (1001, ch)
    assert np.array_equal(got, want.reshape(1001, ch)) and np.array_equal(got, pcm)


def test_other_sample_widths_and_rates_are_refused(tmp_path):
    from vipant_amd._ffi import VipantError
    from vipant_amd.data import ImageAudioSrc, read_wav
    SF.write_wav(f"{tmp_path}/w8.wav", (bytes(range(200)), 1), width=1)
    SF.write_wav(f"{tmp_path}/w24.wav", (bytes(600), 2), width=3)
    with pytest.raises(VipantError, match=r"w8\.wav: 8-bit"):
        read_wav(f"{tmp_path}/w8.wav")
    with pytest.raises(VipantError, match=r"w24\.wav: 24-bit"):
        read_wav(f"{tmp_path}/w24.wav")
    with open(f"{tmp_path}/junk.wav", "wb") as f:
        f.write(b"not a wave file at all")
    with pytest.raises(VipantError, match=r"junk\.wav"):
        read_wav(f"{tmp_path}/junk.wav")
    SF.write_wav(f"{tmp_path}/clip/k.wav", SF.noise_clip(np.random.default_rng(0), 2205, 1), rate=22050)
    SF.write_png(f"{tmp_path}/frame/k.png", np.zeros((8, 9, 3), dtype=np.uint8))
    _index(tmp_path, "src_toy", [{"id": "k", "dir": "", "clip": ["wav"], "frame": "png"}])
    ds = ImageAudioSrc(_rcfg(tmp_path), "src_toy", train=False)
    with pytest.raises(VipantError, match="22050 Hz"):
        ds[0]
    assert ImageAudioSrc(_rcfg(tmp_path, sample_rate=22050), "src_toy", train=False)[0]["pcm"].shape == (2205, 1)


def test_read_frame_and_pluggable_decoders(tmp_path):
    from vipant_amd.data import ImageAudioSrc, read_frame
    fr = np.random.default_rng(1).integers(0, 256, size=(37, 53, 3), dtype=np.int64).astype(np.uint8)
    SF.write_png(f"{tmp_path}/frame/p.png", fr)
    got = read_frame(f"{tmp_path}/frame/p.png")
    assert got.dtype == np.uint8 and np.array_equal(got, fr)
    from PIL import Image
    Image.fromarray(fr[:, :, 0]).save(f"{tmp_path}/gray.png")                         # a grey file becomes three channels
    assert read_frame(f"{tmp_path}/gray.png").shape == (37, 53, 3)
    _index(tmp_path, "src_toy", [{"id": "p", "dir": "", "clip": ["flac"], "frame": "png"}])
    seen = []

    def flac(path):
        seen.append(path)
        return np.arange(12, dtype=np.int16), 16000                                   # a mono decoder may return [n]
    ds = ImageAudioSrc(_rcfg(tmp_path), "src_toy", train=False, decode_audio=flac, decode_frame=lambda p: fr[::-1].copy())
    item = ds[0]
    assert seen == [f"{tmp_path}/clip/p.flac"] and item["pcm"].shape == (12, 1) and np.array_equal(item["frame"], fr[::-1])
    assert item["name"] == "p" and set(item) == {"name", "frame", "pcm"}


# ------------------------------------------------------------------ 3. fallbacks
def test_a_broken_frame_becomes_a_random_frame_and_a_broken_clip_raises(tmp_path):
    from vipant_amd._ffi import VipantError
    from vipant_amd.data import ImageAudioSrc
    SF.make_src_dir(str(tmp_path), "src_toy", [0.01, 0.01], [1, 2], [(8, 9), (8, 9)])
    with open(f"{tmp_path}/frame/c0.png", "wb") as f:
        f.write(b"broken")
    ds = ImageAudioSrc(_rcfg(tmp_path), "src_toy", train=False, seed=3)
    with pytest.warns(UserWarning, match=r"use random image instead because `.*` .*frame/c0\.png\."):
        item = ds[0]
    assert item["frame"].dtype == np.uint8 and item["frame"].shape == (32, 32, 3) and len(np.unique(item["frame"])) > 100
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert np.array_equal(ds[0]["frame"], item["frame"])                        # evaluation: the same frame every time
    with open(f"{tmp_path}/clip/c1.wav", "wb") as f:
        f.write(b"broken")
    with pytest.raises(VipantError, match=r"c1\.wav"):
        ds[1]


def test_frame_embeddings_take_the_image_slot(tmp_path):
    from vipant_amd.data import ImageAudioSrc, SrcCollator
    SF.make_src_dir(str(tmp_path), "src_toy", [0.01, 0.02], [1, 2], [(8, 9), (8, 9)], nframes_per_item=[2, 5])
    v = np.random.default_rng(2).standard_normal((2, 16)).astype(np.float32)
    os.makedirs(f"{tmp_path}/emb")
    np.savez(f"{tmp_path}/emb/c0.000.npz", v=v[0])
    np.savez(f"{tmp_path}/emb/c1.002.npz", v=v[1])
    ds = ImageAudioSrc(_rcfg(tmp_path, frame_emb="emb"), "src_toy", train=False)
    items = [ds[0], ds[1]]
    assert all(set(it) == {"name", "embed", "pcm"} for it in items)
    batch = SrcCollator()(items)
    assert batch[0].dtype == torch.float32 and torch.equal(batch[0], torch.from_numpy(v))
    os.remove(f"{tmp_path}/emb/c1.002.npz")
    with pytest.warns(UserWarning, match="use random image instead"):
        assert ds[1]["embed"].shape == (16,)


# ------------------------------------------------------------------ 4. the collator and the loader
def _toy(tmp_path):
    return SF.make_src_dir(str(tmp_path), "src_toy", [0.011, 0.03, 0.0205625, 0.025, 0.04, 0.002], [1, 2, 6, 2, 1, 2],
                           [(37, 53), (40, 30), (9, 64), (37, 53), (12, 12), (20, 21)], nframes_per_item=[0, 3, 4, 0, 6, 2])


def test_collator_containers(tmp_path):
    from vipant_amd.data import FrameBatch, ImageAudioSrc, PcmBatch, SrcCollator
    records, clips, frames = _toy(tmp_path)
    ds = ImageAudioSrc(_rcfg(tmp_path), "src_toy", train=False)
    images, audios, text, labels, names = SrcCollator(16000)([ds[i] for i in range(6)])
    assert isinstance(images, FrameBatch) and isinstance(audios, PcmBatch) and names == [r["id"] for r in records]
    assert images.frames.dtype == torch.uint8 and images.frames.shape == (6, 40, 64, 3) and images.hw.dtype == torch.int32
    assert images.hw.tolist() == [[37, 53], [40, 30], [9, 64], [37, 53], [12, 12], [20, 21]]
    picks = [0, 1, 1, 0, 2, 0]                                                         # ceil(len / 2) - 1 of 1, 3, 4, 1, 6, 2 frames
    for i, (h, w) in enumerate(images.hw.tolist()):
        assert np.array_equal(images.frames[i, :h, :w].numpy(), frames[i][picks[i]])
        assert int(images.frames[i, h:].sum()) == 0 and int(images.frames[i, :, w:].sum()) == 0
    sizes = [c.size for c in clips]
    assert audios.pcm.dtype == torch.int16 and audios.pcm.shape == (6, -(-max(sizes) // 8) * 8) and audios.pcm.shape[1] % 8 == 0
    assert max(sizes) % 8 != 0                                                         # (the rounding is exercised)
    assert audios.nframes.dtype == torch.int64 and audios.nframes.tolist() == [c.shape[0] for c in clips]
    assert audios.channels.dtype == torch.int32 and audios.channels.tolist() == [1, 2, 6, 2, 1, 2] and audios.sample_rate == 16000
    for i, c in enumerate(clips):
        assert np.array_equal(audios.pcm[i, :c.size].numpy(), c.reshape(-1)) and int(audios.pcm[i, c.size:].abs().sum()) == 0
    assert text.dtype == torch.int64 and text.shape == (6, 1) and not text.any()
    assert labels.dtype == torch.int64 and labels.shape == (6,) and not labels.any()
    for t in (images.frames, images.hw, audios.pcm, audios.nframes, audios.channels, text, labels):
        assert t.device.type == "cpu"
    moved = audios.to("cpu")
    assert isinstance(moved, PcmBatch) and torch.equal(moved.pcm, audios.pcm) and images.to("cpu").hw is images.hw


def _cfg(tmp_path, workers, **kw):
    from vipant_amd.config import to_config
    return to_config({"seed": 1213, "num_proc": workers, "running": dict(_rcfg(tmp_path, **kw))})


def _flat(batch):
    return [batch[0].frames, batch[0].hw, batch[1].pcm, batch[1].nframes, batch[1].channels, batch[2], batch[3]], list(batch[4])


def test_workers_do_not_change_a_batch_and_epochs_change_the_train_draws(tmp_path):
    from vipant_amd.data import build_image_audio_dataloader
    _toy(tmp_path)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                                # (pin_memory without an accelerator)
        _, one = build_image_audio_dataloader(_cfg(tmp_path, 0), "src_toy", shuffle=False, train=True)
        _, two = build_image_audio_dataloader(_cfg(tmp_path, 2), "src_toy", shuffle=False, train=True)
        assert isinstance(one, torch.utils.data.DataLoader) and two.num_workers == 2 and len(one) == 2
        assert two.multiprocessing_context.get_start_method() == "spawn"
        a, b = list(one), list(two)
        assert len(a) == len(b) == 2
        for x, y in zip(a, b):
            (tx, nx), (ty, ny) = _flat(x), _flat(y)
            assert nx == ny and all(torch.equal(p, q) for p, q in zip(tx, ty))
        # training draws (the frame of a list) follow the epoch; evaluation does not
        picks = []
        for epoch in range(6):
            one.dataset.set_epoch(epoch)
            picks.append([one.dataset._process_item(i)[2] for i in range(6)])
        assert len({tuple(p) for p in picks}) > 1
        one.dataset.set_epoch(0)
        assert [one.dataset._process_item(i)[2] for i in range(6)] == picks[0]
        assert all(torch.equal(p, q) for p, q in zip(_flat(next(iter(one)))[0], _flat(a[0])[0]))
        _, ev = build_image_audio_dataloader(_cfg(tmp_path, 0), "src_toy", shuffle=False, train=False)
        first = _flat(next(iter(ev)))[0]
        ev.dataset.set_epoch(3)
        assert all(torch.equal(p, q) for p, q in zip(_flat(next(iter(ev)))[0], first))
        assert isinstance(ev.sampler, torch.utils.data.SequentialSampler)
        _, sh = build_image_audio_dataloader(_cfg(tmp_path, 0), "src_toy", shuffle=True, train=True)
        assert isinstance(sh.sampler, torch.utils.data.RandomSampler)


def test_the_data_package_never_loads_the_binding():
    import subprocess
    code = ("import sys; import vipant_amd.data, cvap.data; assert cvap.data.ImageAudioSrc is vipant_amd.data.ImageAudioSrc; "
            "assert 'vipant_amd._ffi' not in sys.modules and 'vipant_amd.ops' not in sys.modules, sorted(m for m in sys.modules if 'vipant' in m)")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


# ------------------------------------------------------------------ 5. the ABI without a device
def test_pcm_wave_refusals_need_no_device():
    from vipant_amd import _ffi, build
    build.build(verbose=False)
    lib = _ffi.lib()
    assert hasattr(lib, "vipant_pcm_wave")
    assert _ffi.ABI_VERSION == lib.vipant_version() == 101                              # new exports, no bump
    ok = dict(pcm=256, pcm_stride=64, nframes=256, channels=256, mode=0, tile_len=0, wave=256, wave_stride=64, nout=256, b=2)

    def call(**kw):
        a = dict(ok, **kw)
        _ffi.call("vipant_pcm_wave", a["pcm"], a["pcm_stride"], a["nframes"], a["channels"], a["mode"], a["tile_len"], a["wave"],
                  a["wave_stride"], a["nout"], a["b"], None)
    for name in ("pcm", "nframes", "channels", "wave", "nout"):
        with pytest.raises(_ffi.VipantError, match="NULL argument"):
            call(**{name: None})
    with pytest.raises(_ffi.VipantError, match="b = 0"):
        call(b=0)
    with pytest.raises(_ffi.VipantError, match="unknown mode 7"):
        call(mode=7)
    for name in ("pcm_stride", "wave_stride"):
        with pytest.raises(_ffi.VipantError, match="strides"):
            call(**{name: 0})
    with pytest.raises(_ffi.VipantError, match="tile_len"):
        call(tile_len=-1)
