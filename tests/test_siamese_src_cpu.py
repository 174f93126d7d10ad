"""The siamese trainer's raw-file dataset on the host (vipant_amd/data: ImageAudioSiameseSrc, SiameseSrcCollator, SecondView) and the
mask-override form of KaldiFbank.draw_masks.  A generated tree as tests/src_fixture.py makes one; no device."""
import hashlib
import os
import warnings

import numpy as np
import pytest
import torch

import src_fixture as SF

SECONDS = [0.011, 0.03, 0.0205625, 0.025, 0.04, 0.002]
CHANNELS = [1, 2, 6, 2, 1, 2]
FRAMES = [(37, 53), (40, 30), (9, 64), (37, 53), (12, 12), (20, 21)]
NAMES = [0, 3, 4, 0, 6, 2]                    # frame names per item: 0 = the frame is a single name (no embedding file)
PICKS = [0, 1, 1, 0, 2, 0]                    # evaluation: ceil(len / 2) - 1
E = 16


def _toy(tmp_path):
    records, clips, frames = SF.make_src_dir(str(tmp_path), "src_toy", SECONDS, CHANNELS, FRAMES, nframes_per_item=NAMES)
    os.makedirs(f"{tmp_path}/emb", exist_ok=True)
    embeds = np.random.default_rng(2).standard_normal((6, E)).astype(np.float32)
    for i, r in enumerate(records):
        if NAMES[i]:
            np.savez(f"{tmp_path}/emb/{r['id']}.{PICKS[i]:03d}.npz", v=embeds[i])
    return records, clips, frames, embeds


def _cfg(tmp_path, workers=0, vp=True, ap=False, **kw):
    from vipant_amd.config import to_config
    running = dict(data_root=str(tmp_path), eval_samples=5184, train_samples=1.0, frame_key="frame", frame_emb="emb", resolution=32,
                   embed_dim=E, sample_rate=16000, batch_size=3, multi_view=True)
    running.update(kw)
    return to_config({"seed": 1213, "num_proc": workers, "running": running,
                      "model": {"loss": {"vp": vp, "ap": ap, "vv": True, "aa": True, "va": True}}})


def _nbytes(t):
    return t.numel() * t.element_size()


def test_multi_view_selects_the_siamese_dataset_and_frame_emb_is_required(tmp_path):
    from vipant_amd._ffi import VipantError
    from vipant_amd.data import (ImageAudioSiameseSrc, ImageAudioSrc, SiameseSrcCollator, SrcCollator,
                                 build_image_audio_dataloader)
    import cvap.data
    _toy(tmp_path)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                                # (pin_memory without an accelerator)
        _, loader = build_image_audio_dataloader(_cfg(tmp_path), "src_toy", shuffle=False, train=False)
        assert type(loader.dataset) is ImageAudioSiameseSrc and isinstance(loader.collate_fn, SiameseSrcCollator)
        assert isinstance(loader.dataset, ImageAudioSrc) and cvap.data.ImageAudioSiameseSrc is ImageAudioSiameseSrc
        _, plain = build_image_audio_dataloader(_cfg(tmp_path, multi_view=False), "src_toy", shuffle=False, train=False)
        assert type(plain.dataset) is ImageAudioSrc and isinstance(plain.collate_fn, SrcCollator)
    with pytest.raises(VipantError, match="running.frame_emb"):
        build_image_audio_dataloader(_cfg(tmp_path, frame_emb=None), "src_toy", shuffle=False, train=False)
    with pytest.raises(VipantError, match="running.frame_emb"):
        ImageAudioSiameseSrc(_cfg(tmp_path, frame_emb=None), "src_toy", train=True)


@pytest.mark.parametrize("vp,ap", [(True, False), (False, True), (False, False)])
def test_items_and_the_six_slots(tmp_path, vp, ap):
    from vipant_amd.data import FrameBatch, ImageAudioSiameseSrc, PcmBatch, SecondView, SiameseSrcCollator
    records, clips, frames, embeds = _toy(tmp_path)
    ds = ImageAudioSiameseSrc(_cfg(tmp_path, vp=vp, ap=ap), "src_toy", train=False)
    listed = [i for i in range(6) if NAMES[i]]
    items = [ds[i] for i in listed]
    for i, it in zip(listed, items):
        assert set(it) == ({"name", "frame", "pcm", "embed"} if vp or ap else {"name", "frame", "pcm"})
        assert it["frame"].dtype == np.uint8 and np.array_equal(it["frame"], frames[i][PICKS[i]])
        assert it["pcm"].dtype == np.int16 and np.array_equal(it["pcm"], clips[i]) and it["name"] == records[i]["id"]
        if vp or ap:
            assert it["embed"].dtype == np.float32 and np.array_equal(it["embed"], embeds[i])
    batch = SiameseSrcCollator(16000)(items)
    assert len(batch) == 6 and batch[5] == [records[i]["id"] for i in listed]
    image, image_v1, image_v2, audio_v1, audio_v2, _ = batch
    if vp or ap:
        assert image.dtype == torch.float32 and torch.equal(image, torch.from_numpy(embeds[listed]))
    else:
        assert image.dtype == torch.float32 and image.shape == (4, 1, 1, 1) and bool((image == 1).all())
    assert isinstance(image_v1, FrameBatch) and isinstance(audio_v1, PcmBatch)
    assert image_v1.frames.dtype == torch.uint8 and image_v1.frames.shape == (4, 40, 64, 3)
    assert image_v1.hw.tolist() == [list(FRAMES[i]) for i in listed]
    assert audio_v1.pcm.dtype == torch.int16 and audio_v1.nframes.tolist() == [clips[i].shape[0] for i in listed]
    assert audio_v1.channels.tolist() == [CHANNELS[i] for i in listed] and audio_v1.sample_rate == 16000
    # the second view slots name the slot they are a view of and hold nothing
    assert isinstance(image_v2, SecondView) and image_v2.of == 1 and isinstance(audio_v2, SecondView) and audio_v2.of == 3
    assert not any(isinstance(v, torch.Tensor) for m in (image_v2, audio_v2) for v in vars(m).values())
    assert image_v2.to("cpu") is image_v2 and audio_v2.pin_memory() is audio_v2
    tensors = [image, image_v1.frames, image_v1.hw, audio_v1.pcm, audio_v1.nframes, audio_v1.channels]
    tensors += [v for m in (image_v2, audio_v2) for v in vars(m).values() if isinstance(v, torch.Tensor)]
    payload = (_nbytes(image_v1.frames) + _nbytes(image_v1.hw)) + (_nbytes(audio_v1.pcm) + _nbytes(audio_v1.nframes)
                                                                 + _nbytes(audio_v1.channels)) + _nbytes(image)
    assert sum(_nbytes(t) for t in tensors) == payload
    assert payload == 4 * 40 * 64 * 3 + 4 * 2 * 4 + audio_v1.pcm.shape[1] * 4 * 2 + 4 * 8 + 4 * 4 + (4 * E * 4 if vp or ap else 4 * 4)


def test_a_single_name_frame_gets_the_warned_random_embedding(tmp_path):
    from vipant_amd.data import ImageAudioSiameseSrc
    _toy(tmp_path)
    ds = ImageAudioSiameseSrc(_cfg(tmp_path), "src_toy", train=False)
    assert ds._process_item(0)[3] is None                                          # a single name: no embedding file
    with pytest.warns(UserWarning, match="use random image instead because"):
        item = ds[0]
    assert set(item) == {"name", "frame", "pcm", "embed"} and item["embed"].shape == (E,) and item["embed"].dtype == np.float32
    assert 0.0 <= float(item["embed"].min()) and float(item["embed"].max()) < 1.0 and len(np.unique(item["embed"])) == E
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert np.array_equal(ds[0]["embed"], item["embed"])                       # evaluation: the same vector every time
    quiet = ImageAudioSiameseSrc(_cfg(tmp_path, vp=False, ap=False), "src_toy", train=False)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                             # nobody reads the embedding: nothing is loaded
        assert set(quiet[0]) == {"name", "frame", "pcm"}


def _flat(batch):
    return [batch[0], batch[1].frames, batch[1].hw, batch[3].pcm, batch[3].nframes, batch[3].channels], list(batch[5])


def test_the_batch_survives_a_spawned_worker(tmp_path):
    from vipant_amd.data import FrameBatch, PcmBatch, SecondView, build_image_audio_dataloader
    _toy(tmp_path)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, here = build_image_audio_dataloader(_cfg(tmp_path, 0), "src_toy", shuffle=False, train=True)
        _, there = build_image_audio_dataloader(_cfg(tmp_path, 1), "src_toy", shuffle=False, train=True)
        assert there.num_workers == 1 and there.multiprocessing_context.get_start_method() == "spawn"
        a, b = list(here), list(there)
    assert len(a) == len(b) == 2
    for x, y in zip(a, b):
        assert isinstance(y[1], FrameBatch) and isinstance(y[3], PcmBatch) and y[3].sample_rate == 16000
        assert isinstance(y[2], SecondView) and y[2].of == 1 and isinstance(y[4], SecondView) and y[4].of == 3
        (tx, nx), (ty, ny) = _flat(x), _flat(y)
        assert nx == ny and all(p.dtype == q.dtype and torch.equal(p, q) for p, q in zip(tx, ty))


# sha256 of KaldiFbank(16000, 64, 256, freq_mask_param=32, time_mask_param=200).draw_masks(6, Generator().manual_seed(3)) as int32
# bytes, and of the next torch.rand(4) of that generator, recorded from the parent commit
PARENT_MASKS = "181810f6ea2410b2924baba1bb0f90cb26114b01fe70275806715c35d9367520"
PARENT_NEXT = "416c68c663f69e4f9fccf9775e97e5c7dae289210d65e8b36efc97e304e37199"


def _digest(t):
    return hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest()


def test_mask_overrides_consume_the_generator_as_the_default_form_does():
    from vipant_amd.frontend import KaldiFbank
    own = KaldiFbank(16000, 64, 256, freq_mask_param=32, time_mask_param=200, device="cpu")
    g = torch.Generator().manual_seed(3)
    masks = own.draw_masks(6, g)
    assert masks.dtype == torch.int32 and masks.shape == (6, 4)
    assert _digest(masks) == PARENT_MASKS and _digest(torch.rand(4, generator=g)) == PARENT_NEXT
    # the override form on an object without masks of its own: the same draws, the same generator state afterwards
    bare = KaldiFbank(16000, 64, 256, device="cpu")
    assert bare.draw_masks(6, torch.Generator().manual_seed(3)) is None
    g = torch.Generator().manual_seed(3)
    assert torch.equal(bare.draw_masks(6, g, freq_mask_param=32, time_mask_param=200), masks)
    assert _digest(torch.rand(4, generator=g)) == PARENT_NEXT
    # two sets from one object, one after the other: the second set continues where the first stopped
    g, h = torch.Generator().manual_seed(3), torch.Generator().manual_seed(3)
    prime = bare.draw_masks(6, g, freq_mask_param=32, time_mask_param=200)
    second = bare.draw_masks(6, g, freq_mask_param=48, time_mask_param=300)
    wide = KaldiFbank(16000, 64, 256, freq_mask_param=48, time_mask_param=300, device="cpu")
    assert torch.equal(prime, own.draw_masks(6, h)) and torch.equal(second, wide.draw_masks(6, h))
    assert torch.equal(torch.rand(4, generator=g), torch.rand(4, generator=h))
    assert int((second[:, 1] - second[:, 0]).max()) < 48 and int((second[:, 3] - second[:, 2]).max()) < 300
    # one override only: the other parameter stays the object's
    g = torch.Generator().manual_seed(3)
    assert torch.equal(own.draw_masks(6, g, time_mask_param=200), masks)
    assert own.draw_masks(2, torch.Generator().manual_seed(3), freq_mask_param=0, time_mask_param=0) is None


def test_pair_entry_refusals_need_no_device():
    from vipant_amd import _ffi, build
    build.build(verbose=False)
    lib = _ffi.lib()
    assert hasattr(lib, "vipant_fbank_view_pair")
    assert _ffi.ABI_VERSION == lib.vipant_version() == 101                              # a new export, no bump
    b, T, F = 2, 8, 16
    n = b * T * F * 4
    params = _ffi.ViewParams(0, 0, 2000, 0, 0.0, 0, 1, 1, 0, 0)
    ok = dict(out=4096, out2=4096 + n, ws=256, wsb=_ffi.query("vipant_fbank_view_workspace_bytes", b), draws=256)

    def call(**kw):
        a = dict(ok, **kw)
        _ffi.call("vipant_fbank_view_pair", 256, 4000, 256, a["out"], a["out2"], 256, 256, 256, 256, None, None, b, T, F, 400, 160, 512,
                  0.97, 0.0, 0.0, params, a["draws"], a["ws"], a["wsb"], None)
    with pytest.raises(_ffi.VipantError, match="fbank_view_pair: null second output"):
        call(out2=None)
    for out2 in (4096, 4096 + n - 4, 4096 - n + 4):
        with pytest.raises(_ffi.VipantError, match="fbank_view_pair: the two outputs overlap"):
            call(out2=out2)
    with pytest.raises(_ffi.VipantError, match="fbank_view_pair: null argument"):
        call(out=None)
    with pytest.raises(_ffi.VipantError, match="fbank_view_pair: null argument"):
        call(draws=None)
    with pytest.raises(_ffi.VipantError, match="fbank_view_pair: workspace too small"):
        call(wsb=ok["wsb"] - 1)
