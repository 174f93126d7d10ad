"""The caption datasets on the host (vipant_amd/data/audio_text.py): index, path, frame and text rules against what the reference's
own `AudioCapDatasetSrc._process_item`, text collator and `build_clotho_data_list` recorded (tests/golden/audiocaps_dataset.json, made
by tests/golden/make_golden_audiocaps.py), the caption draws, the truncation rules, the refusals and worker independence."""
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import at_fixture as AF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "audiocaps_dataset.json")))
SECONDS = [0.011, 0.03, 0.0205, 0.025, 0.04, 0.002]
CHANNELS = [1, 2, 1, 2, 1, 2]


def _rcfg(root, **kw):
    from vipant_amd.config import to_config
    base = dict(data_root=str(root), eval_samples=5184, train_samples=1.0, frame_key="frame", frame_emb=None, resolution=32, embed_dim=16,
                sample_rate=16000, batch_size=4, imagine=False, clf=False, prompt="", bpe_path=AF.BPE, clip_model_root="/nonexistent")
    base.update(kw)
    return to_config(base)


def _cfg(root, workers=0, **kw):
    from vipant_amd.config import to_config
    return to_config({"seed": 1213, "num_proc": workers, "running": dict(_rcfg(root, **kw))})


# ------------------------------------------------------------------ 1. against the reference's record
@pytest.mark.parametrize("case", range(len(GOLD["cases"])))
def test_paths_frames_and_evaluation_text_are_the_reference_s(tmp_path, case):
    from vipant_amd.data import AudioCapSrc
    c = GOLD["cases"][case]
    records = [{(c["clip_key"] if k == "clip" else k): v for k, v in r.items()} for r in GOLD["records"]]
    assert len(records) == 6 and sorted(len(r["captions"]) for r in records) == [1, 1, 5, 5, 5, 5]
    assert [r["frame"] if isinstance(r["frame"], str) else len(r["frame"]) for r in records] == ["png", 1, 2, 5, "jpg", 5]
    AF.write_index(tmp_path, "audiocaps_toy", records)
    ds = AudioCapSrc(_rcfg(tmp_path, imagine=c["imagine"], frame_emb=c["frame_emb"]), "audiocaps_toy", train=False)
    assert ds.aclip_key == c["clip_key"] and len(ds) == 6
    for i, want in enumerate(c["items"]):
        name, text, clip_file, frame_file, embed_file = ds._caption_item(i)
        rebase = lambda v: None if v is None else v.replace("ROOT", str(tmp_path), 1)
        assert (name, clip_file, frame_file, embed_file) == (want["name"], rebase(want["clip_file"]), rebase(want["frame_file"]),
                                                             rebase(want["frame_emb_file"])), (i, want)
        assert text == want["text"] and len(text) == len(records[i]["captions"])
    if not c["imagine"]:
        assert all(it["frame_file"] is None and it["frame_emb_file"] is None for it in c["items"])


def test_collated_text_is_the_reference_collator_s_array(tmp_path):
    from vipant_amd.data import AudioCapSrc, CaptionCollator, FrameBatch, PcmBatch, collate_text
    records, clips, _ = AF.make_audiocaps_dir(str(tmp_path), "audiocaps_toy", SECONDS, CHANNELS)
    for r, g in zip(records, GOLD["records"]):
        r["captions"] = g["captions"]
    AF.write_index(tmp_path, "audiocaps_toy", records)
    ds = AudioCapSrc(_rcfg(tmp_path), "audiocaps_toy", train=False)
    items = [ds[i] for i in range(6)]
    assert all(set(it) == {"name", "text", "pcm"} for it in items)
    want = GOLD["collated"]["train"]
    train_items = [dict(it, text=it["text"][p]) for it, p in zip(items, want["pick"])]
    images, audios, text, labels, names = CaptionCollator(16000)(train_items)
    assert text.dtype == torch.int64 and text.tolist() == want["text"] and names == [r["id"] for r in records]
    assert text.shape == (6, max(len(it["text"]) for it in train_items))
    for row, it in zip(text.tolist(), train_items):
        n = len(it["text"])
        assert row[:n] == it["text"] and row[n - 1] == 49407 and not any(row[n:])
    assert images.dtype == torch.float32 and images.shape == (6, 1, 1, 1) and bool((images == 1).all())
    assert isinstance(audios, PcmBatch) and audios.nframes.tolist() == [c.shape[0] for c in clips] and audios.channels.tolist() == CHANNELS
    for i, c in enumerate(clips):
        assert np.array_equal(audios.pcm[i, :c.size].numpy(), c.reshape(-1))
    assert labels.dtype == torch.int64 and labels.shape == (6,) and not labels.any()
    # evaluation: every caption, a clip's captions contiguous in clip order
    want = GOLD["collated"]["eval"]
    picked = [items[i] for i in want["eval_records"]]
    images, audios, text, labels, names = CaptionCollator(16000)(picked)
    assert text.dtype == torch.int64 and text.tolist() == want["text"] and text.shape[0] == 20 == sum(len(it["text"]) for it in picked)
    assert text.shape[1] == max(len(row) for it in picked for row in it["text"]) < 77
    k = 0
    for it in picked:                                                                  # a clip's captions are contiguous, in clip order
        for row in it["text"]:
            assert text[k, :len(row)].tolist() == row and not text[k, len(row):].any()
            k += 1
    assert len(names) == 4 == labels.shape[0] == images.shape[0] == audios.pcm.shape[0]
    # a record with one caption among records with five
    mixed = CaptionCollator(16000)(items)[2]
    assert mixed.shape[0] == 22
    with pytest.raises(ValueError, match="unrecognized"):
        collate_text([["a"]])
    # frames and embeddings take the image slot under `imagine`
    _, _, frames = AF.make_audiocaps_dir(str(tmp_path), "audiocaps_img", SECONDS[:2], CHANNELS[:2], frame_hw=[(8, 9), (12, 7)],
                                         nframes_per_item=[0, 3])
    ds = AudioCapSrc(_rcfg(tmp_path, imagine=True), "audiocaps_img", train=False)
    batch = CaptionCollator(16000)([ds[0], ds[1]])
    assert isinstance(batch[0], FrameBatch) and batch[0].hw.tolist() == [[8, 9], [12, 7]]
    assert np.array_equal(batch[0].frames[1, :12, :7].numpy(), frames[1][1]) and batch[2].shape[0] == 10


# ------------------------------------------------------------------ 2. the caption draws
def test_training_captions_follow_seed_index_and_epoch(tmp_path):
    from vipant_amd.data import AudioCapSrc
    records, _, _ = AF.make_audiocaps_dir(str(tmp_path), "audiocaps_toy", SECONDS, CHANNELS, ncaptions=[5, 1, 5, 5, 1, 5])
    ds = AudioCapSrc(_rcfg(tmp_path), "audiocaps_toy", train=True, seed=7)
    same = AudioCapSrc(_rcfg(tmp_path), "audiocaps_toy", train=True, seed=7)
    other = AudioCapSrc(_rcfg(tmp_path), "audiocaps_toy", train=True, seed=8)
    bpe = [r["captions_bpe"] for r in ds.dataset]
    assert [len(b) for b in bpe] == [5, 1, 5, 5, 1, 5]
    drawn, drawn_other = {i: [] for i in range(6)}, {i: [] for i in range(6)}
    for epoch in range(40):
        for d in (ds, same, other):
            d.set_epoch(epoch)
        for i in range(6):
            item = ds[i]
            assert set(item) == {"name", "text", "pcm"} and item["text"] in bpe[i] and isinstance(item["text"][0], int)
            assert same[i]["text"] == item["text"] == ds[i]["text"]
            drawn[i].append(bpe[i].index(item["text"]))
            drawn_other[i].append(bpe[i].index(other[i]["text"]))
    for i in (0, 2, 3, 5):
        assert set(drawn[i]) == {0, 1, 2, 3, 4}, (i, drawn[i])         # every caption of a 5-caption record is drawn
        assert len(set(drawn[i][:8])) > 1                                # and the draw differs across epochs
        assert drawn[i] != drawn_other[i]                                # and with the seed
    assert drawn[1] == [0] * 40
    ds.set_epoch(3)
    assert [bpe[i].index(ds[i]["text"]) for i in range(6)] == [drawn[i][3] for i in range(6)]


def test_rnd_cap_draws_from_other_records(tmp_path):
    from vipant_amd.data import AudioCapSrc
    AF.make_audiocaps_dir(str(tmp_path), "audiocaps_toy", SECONDS, CHANNELS)
    ds = AudioCapSrc(_rcfg(tmp_path, rnd_cap=True), "audiocaps_toy", train=True, seed=7)
    assert ds.rnd_cap and not AudioCapSrc(_rcfg(tmp_path), "audiocaps_toy", train=True).rnd_cap
    every = [row for r in ds.dataset for row in r["captions_bpe"]]
    foreign = 0
    for epoch in range(4):
        ds.set_epoch(epoch)
        for i in range(6):
            text = ds[i]["text"]
            assert text in every and ds[i]["text"] == text
            foreign += text not in ds.dataset[i]["captions_bpe"]
    assert foreign >= 12                                # 5 of 6 records are other records: about 20 of the 24 draws
    ev = AudioCapSrc(_rcfg(tmp_path, rnd_cap=True), "audiocaps_toy", train=False)
    assert ev[2]["text"] == ev.dataset[2]["captions_bpe"]                   # a training rule


def test_the_frame_draw_comes_before_the_caption_draw(tmp_path):
    from vipant_amd.data import AudioCapSrc
    AF.make_audiocaps_dir(str(tmp_path), "audiocaps_toy", SECONDS[:2], CHANNELS[:2], frame_hw=[(8, 9), (8, 9)], nframes_per_item=[5, 5])
    ds = AudioCapSrc(_rcfg(tmp_path, imagine=True, rnd_cap=True), "audiocaps_toy", train=True, seed=3)
    ds.set_epoch(2)
    g = torch.Generator().manual_seed(3 + 13 + 1 + 1000003 * 2)
    frame = int(torch.randint(5, (1,), generator=g))
    record = int(torch.randint(2, (1,), generator=g))
    caption = int(torch.randint(5, (1,), generator=g))
    name, text, clip_file, frame_file, embed_file = ds._caption_item(1)
    assert frame_file == f"{tmp_path}/frame/y1.{frame:03d}.png" and text == ds.dataset[record]["captions_bpe"][caption]
    assert set(ds[1]) == {"name", "text", "pcm", "frame"} and ds[1]["frame"].shape == (8, 9, 3)
    # nothing imagined: the frame is not drawn, the same generator gives record and caption first
    plain = AudioCapSrc(_rcfg(tmp_path, imagine=False, rnd_cap=True), "audiocaps_toy", train=True, seed=3)
    plain.set_epoch(2)
    g = torch.Generator().manual_seed(3 + 13 + 1 + 1000003 * 2)
    record = int(torch.randint(2, (1,), generator=g))
    caption = int(torch.randint(5, (1,), generator=g))
    assert plain._caption_item(1)[1] == plain.dataset[record]["captions_bpe"][caption] and plain._caption_item(1)[3] is None


# ------------------------------------------------------------------ 3. truncation and refusals
def test_truncation_fraction_and_refusals(tmp_path):
    from vipant_amd.data import AudioCapSrc, AudioTextSrc, build_audio_text_dataloader, build_audiocaps_data_list
    from vipant_amd.errors import VipantError
    records = [{"id": f"r{i}", "dir": "", "clip": ["wav"], "frame": "png", "labels": [], "captions": [f"clip number {i}"]} for i in range(20)]
    AF.write_index(tmp_path, "audiocaps_toy", records)
    assert len(AudioCapSrc(_rcfg(tmp_path, eval_samples=5), "audiocaps_toy", train=False)) == 5
    assert len(AudioCapSrc(_rcfg(tmp_path, eval_samples=5), "audiocaps_toy", train=True)) == 20
    half = AudioCapSrc(_rcfg(tmp_path, train_samples=0.5), "audiocaps_toy", train=True, seed=4)
    same = AudioCapSrc(_rcfg(tmp_path, train_samples=0.5), "audiocaps_toy", train=True, seed=4)
    ids = [r["id"] for r in half.dataset]
    assert len(ids) == 10 == len(set(ids)) and ids == [r["id"] for r in same.dataset] and ids != [f"r{i}" for i in range(10)]
    assert all("captions_bpe" in r for r in half.dataset)
    assert len(AudioCapSrc(_rcfg(tmp_path, train_samples=0.5), "audiocaps_toy", train=False)) == 20
    with pytest.raises(VipantError, match="running.clf=True"):
        AudioCapSrc(_rcfg(tmp_path, clf=True), "audiocaps_toy", train=True)
    with pytest.raises(VipantError, match=r"audiocaps_none\.csv is not a file\."):
        AudioCapSrc(_rcfg(tmp_path), "audiocaps_none", train=True)
    with pytest.raises(ValueError, match=r"^unrecognized dataset `esc50`\.$"):
        build_audio_text_dataloader(_cfg(tmp_path), "esc50", shuffle=False, train=False)
    with pytest.raises(VipantError, match=r"running\.bpe_path"):
        AudioCapSrc(_rcfg(tmp_path, bpe_path=""), "audiocaps_toy", train=True)
    # the AudioCaps index as an audio-text list: the prompt goes in front, the clip is read by the AudioCaps path rule
    lst = build_audiocaps_data_list(_rcfg(tmp_path, prompt=" the sound of "), "audiocaps_toy")
    assert lst[3]["label_str"] == ["the sound of clip number 3"] and lst[3]["label_int_bpe"][0][1:4] == [518, 3608, 539]
    ds = AudioTextSrc(_rcfg(tmp_path, eval_samples=7), lst, train=False)
    assert len(ds) == 7 and ds._caption_item(3)[2] == f"{tmp_path}/clip/r3.wav" and len(AudioTextSrc(_rcfg(tmp_path), lst, train=True)) == 20
    with pytest.raises(VipantError, match="running.clf=True"):
        AudioTextSrc(_rcfg(tmp_path, clf=True), lst, train=True)


def test_clotho_lists_are_the_reference_s(tmp_path):
    from vipant_amd.data import AudioTextSrc, build_audio_text_dataloader, build_clotho_data_list
    assert [lst["prompt"].strip() for lst in GOLD["clotho"]["lists"]] == ["", "the sound of"]
    for lst in GOLD["clotho"]["lists"]:
        with open(f"{tmp_path}/{lst['data_name']}.csv", "w") as f:
            f.write(GOLD["clotho"]["csv"])
        got = build_clotho_data_list(_rcfg(tmp_path, prompt=lst["prompt"]), lst["data_name"])
        assert got == lst["records"] and len(got) == 3 and all(r["dir"] == "development" and r["aclip"] == [r["id"]] for r in got)
    ds = AudioTextSrc(_rcfg(tmp_path), got, train=False)
    assert ds.aclip_key == "aclip" and ds._caption_item(1)[2] == f"{tmp_path}/development/rain_01.wav"
    # a comma-separated data name concatenates the lists; the clips are the files themselves, at their own rate
    rows, clips = AF.make_clotho_dir(str(tmp_path), "validation", [0.01, 0.02], rate=44100, channels=[1, 2])
    rows2, _ = AF.make_clotho_dir(str(tmp_path), "evaluation", [0.015], rate=44100)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                                # (pin_memory without an accelerator)
        _, loader = build_audio_text_dataloader(_cfg(tmp_path, sample_rate=44100, prompt="the sound of"),
                                                "clotho_validation,clotho_evaluation", shuffle=False, train=False)
        assert len(loader.dataset) == 3 and [r["dir"] for r in loader.dataset.dataset] == ["validation", "validation", "evaluation"]
        images, audios, text, labels, names = next(iter(loader))
    assert names == [r["file_name"] for r in rows + rows2] and text.shape[0] == 15 and audios.sample_rate == 44100
    assert audios.nframes.tolist() == [441, 882, 662] and audios.channels.tolist() == [1, 2, 1]
    assert np.array_equal(audios.pcm[1, :clips[1].size].numpy(), clips[1].reshape(-1))
    assert all(row[:4] == [49406, 518, 3608, 539] for row in text.tolist())
    from vipant_amd.errors import VipantError
    with pytest.raises(VipantError, match="44100 Hz"):
        build_audio_text_dataloader(_cfg(tmp_path), "clotho_validation", shuffle=False, train=False)[1].dataset[0]


# ------------------------------------------------------------------ 4. the package and the loader
def test_the_data_package_never_loads_the_binding():
    code = ("import sys; import vipant_amd.data, cvap.data; assert cvap.data.AudioCapSrc is vipant_amd.data.AudioCapSrc; "
            "assert cvap.data.build_audio_text_dataloader is vipant_amd.data.build_audio_text_dataloader; "
            "assert 'vipant_amd._ffi' not in sys.modules and 'vipant_amd.ops' not in sys.modules, sorted(m for m in sys.modules if 'vipant' in m)")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


def _flat(batch):
    return [batch[0], batch[1].pcm, batch[1].nframes, batch[1].channels, batch[2], batch[3]], list(batch[4])


@pytest.mark.parametrize("train", [True, False])
def test_workers_do_not_change_a_batch(tmp_path, train):
    from vipant_amd.data import build_audio_text_dataloader
    AF.make_audiocaps_dir(str(tmp_path), "audiocaps_toy", SECONDS, CHANNELS)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                                # (pin_memory without an accelerator)
        _, one = build_audio_text_dataloader(_cfg(tmp_path, 0), "audiocaps_toy", shuffle=False, train=train)
        _, two = build_audio_text_dataloader(_cfg(tmp_path, 2), "audiocaps_toy", shuffle=False, train=train)
        assert isinstance(one, torch.utils.data.DataLoader) and two.num_workers == 2 and len(one) == 2
        assert two.multiprocessing_context.get_start_method() == "spawn"
        assert isinstance(one.sampler, torch.utils.data.SequentialSampler)
        a, b = list(one), list(two)
    assert len(a) == len(b) == 2
    for x, y in zip(a, b):
        (tx, nx), (ty, ny) = _flat(x), _flat(y)
        assert nx == ny and all(torch.equal(p, q) for p, q in zip(tx, ty))
    assert [x[2].shape[0] for x in a] == ([4, 2] if train else [20, 10])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, sh = build_audio_text_dataloader(_cfg(tmp_path, 0), "audiocaps_toy", shuffle=True, train=True)
    assert isinstance(sh.sampler, torch.utils.data.RandomSampler)
