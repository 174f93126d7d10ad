"""The classification datasets on the host (vipant_amd/data/classify.py) against what the reference's own x-fold builders, label
map, filter set and `AudiosetSrc` recorded (tests/golden/clf_dataset.json, made by tests/golden/make_golden_clf_dataset.py); the
tagging batch layout, the per-item mixup draws, worker independence, the weighted sampler and the refusals."""
import contextlib
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import clf_fixture as CF

ROOT = CF.ROOT
GOLD = CF.GOLD


def _cfg(root, workers=0, seed=1213, **kw):
    from vipant_amd.config import to_config
    running = dict(data_root=str(root), data_name="esc50", eval_samples=250000, sample_rate=16000, batch_size=4, prompt="",
                   bpe_path=CF.BPE, clip_model_root="/nonexistent", clf=True, imagine=False, cat_label=False, text_emb=None,
                   force_npz=False, mixup_rate=0.0, weighted_sampling=False, label_map="ontology,eval_segments", filter_set=None,
                   audio={"eval_norms": False})
    running.update(kw)
    return to_config({"seed": seed, "num_proc": workers, "running": running})


@contextlib.contextmanager
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                                # (pin_memory without an accelerator)
        yield


# ------------------------------------------------------------------ 1. the x-fold builders against the reference's record
@pytest.mark.parametrize("which,data_name,nfold", [("esc50", "esc50", 5), ("us8k", "UrbanSound8K", 10)])
@pytest.mark.parametrize("case", range(3))
def test_xfold_lists_prompts_and_label_map_are_the_reference_s(tmp_path, which, data_name, nfold, case):
    from vipant_amd.data import build_xfold_dataloader_list
    c = GOLD[which]["cases"][case]
    assert [x["prompt"] for x in GOLD[which]["cases"]] == ["the sound of", "", "ensemble"]
    (CF.make_esc50_dir if which == "esc50" else CF.make_us8k_dir)(str(tmp_path), ensemble=True)
    shown = []
    loader_list, lid2str, lid2int, label_map = build_xfold_dataloader_list(_cfg(tmp_path, data_name=data_name, prompt=c["prompt"]),
                                                                           echo=shown.append)
    assert len(loader_list) == nfold == len(c["folds"])
    assert {str(k): v for k, v in lid2str.items()} == c["lid2str"] and any("_" in v for v in lid2str.values())
    assert shown == [f"{c['prompts']}"]                                               # prompt strings, `_` replaced by a space
    assert isinstance(lid2int, np.ndarray) and lid2int.tolist() == c["lid2int"]
    assert (None if label_map is None else {str(k): v for k, v in label_map.items()}) == c["label_map"]
    if which == "esc50" and c["prompt"] == "ensemble":
        assert len(lid2int) == 4 * len(lid2str) and all(label_map[i] == i // 4 for i in range(len(lid2int)))
        assert c["prompts"][0] == "the sound of a dog" and not any(p.startswith("a photo of") for p in c["prompts"])
    if which == "us8k":
        assert label_map is None
    # the loaders are lazy: a pair of callables whose closed-over lists are the reference's; nothing was read so far
    for (train_fn, eval_fn), want in zip(loader_list, c["folds"]):
        assert callable(train_fn) and callable(eval_fn)
        assert train_fn.__defaults__[0] == want["train"] and eval_fn.__defaults__[0] == want["eval"]
    with _quiet():
        for k in (0, nfold - 1):
            (_, train), (_, evl) = loader_list[k][0](), loader_list[k][1]()
            held = [r["aclip"] for r in evl.dataset.dataset]
            assert held == [r["aclip"] for r in c["folds"][k]["eval"]] and len(held) == 2
            assert not set(held) & {r["aclip"] for r in train.dataset.dataset} and len(train.dataset) == 2 * (nfold - 1)
            assert isinstance(train.sampler, torch.utils.data.RandomSampler) and isinstance(evl.sampler, torch.utils.data.SequentialSampler)
            assert train.dataset.train and not evl.dataset.train


def test_xfold_items_collation_eval_samples_and_rate(tmp_path):
    from vipant_amd.data import PcmBatch, XFoldCollator, XFoldSrc, build_xfold_dataloader_list
    from vipant_amd.errors import VipantError
    clips = CF.make_esc50_dir(str(tmp_path))
    cfg = _cfg(tmp_path, prompt="the sound of", batch_size=3)
    loader_list, lid2str, _, _ = build_xfold_dataloader_list(cfg, echo=lambda s: None)
    with _quiet():
        _, evl = loader_list[2][1]()
        item = evl.dataset[1]
        assert set(item) == {"pcm", "label_int", "label_str"} and item["pcm"].dtype == np.int16 and item["pcm"].ndim == 2
        rec = evl.dataset.dataset[1]
        assert np.array_equal(item["pcm"], clips[rec["aclip"]]) and lid2str[item["label_int"]] == item["label_str"]
        _, train = loader_list[2][0]()
        batches = list(train)
    assert [b[1].shape[0] for b in batches] == [3, 3, 2]
    audios, labels, names = batches[0]
    assert isinstance(audios, PcmBatch) and audios.sample_rate == 16000 and labels.dtype == torch.int64
    assert names == [lid2str[int(t)] for t in labels]
    assert audios.pcm.dtype == torch.int16 and audios.pcm.shape[1] % 8 == 0
    with _quiet():
        audios, labels, names = next(iter(evl))                                        # sequential: the held-out fold in file order
    for i, rec in enumerate(evl.dataset.dataset):
        c = clips[rec["aclip"]]
        assert (int(audios.nframes[i]), int(audios.channels[i]), int(labels[i]), names[i]) == (c.shape[0], c.shape[1], rec["label_int"],
                                                                                                rec["label_str"])
        assert np.array_equal(audios.pcm[i, :c.size].numpy(), c.reshape(-1))
    full = loader_list[0][0].__defaults__[0]
    assert len(XFoldSrc(cfg.running, full, train=True)) == 8
    cut = _cfg(tmp_path, eval_samples=3).running
    assert len(XFoldSrc(cut, full, train=False)) == 3 and len(XFoldSrc(cut, full, train=True)) == 8
    batch = XFoldCollator(16000)([evl.dataset[0], evl.dataset[1]])
    assert batch[1].tolist() == [evl.dataset.dataset[0]["label_int"], evl.dataset.dataset[1]["label_int"]]
    with pytest.raises(VipantError, match="running.sample_rate = 44100"):
        XFoldSrc(_cfg(tmp_path, sample_rate=44100).running, full, train=True)[0]


# ------------------------------------------------------------------ 2. AudioSet label map, filter set, index reading, items
def test_label_map_and_filter_sets_are_the_reference_s(tmp_path):
    from vipant_amd.data import build_audioset_label_map, build_filter_set
    from vipant_amd.tokenizer import load_tokenizer
    CF.write_audioset_meta(str(tmp_path))
    assert len(GOLD["audioset"]["ontology"]) == 8
    tok = load_tokenizer(CF.BPE)
    for rec in GOLD["audioset"]["label_maps"]:
        got = build_audioset_label_map(str(tmp_path), "ontology,eval_segments", rec["prompt"], tokenizer=tok)
        assert {k: list(v) for k, v in got.items()} == rec["label_map"] and len(got) == 5
        assert list(got) == list(rec["label_map"]) and all(isinstance(v, tuple) for v in got.values())
    assert "/m/0d" not in got                                                         # only a clip's FIRST row is read
    by_rcfg = build_audioset_label_map(str(tmp_path), "ontology,eval_segments", rec["prompt"], rcfg=_cfg(tmp_path).running)
    assert by_rcfg == got
    forms = GOLD["audioset"]["filters"]
    assert sum(f["samples"] is None for f in forms) == 4 and len(forms) == 8
    for f in forms:
        got_set = build_filter_set(str(tmp_path), f["filter_set"])
        assert (None if got_set is None else sorted(got_set)) == f["samples"], f


@pytest.mark.parametrize("case", range(2))
def test_tagging_items_weights_and_index_reading_are_the_reference_s(tmp_path, case):
    from vipant_amd.data import AudiosetSrc
    c = GOLD["tagging"]["cases"][case]
    label_map = {k: tuple(v) for k, v in GOLD["audioset"]["label_maps"][1]["label_map"].items()}
    records, clips = CF.make_audioset_dir(str(tmp_path), clip_key=c["clip_key"])
    assert records == c["records"] and any(len(set(r["labels"])) < len(r["labels"]) for r in records)
    assert {bool(r["dir"]) for r in records} == {True, False}
    rcfg = _cfg(tmp_path, prompt="the sound of").running
    shown = []
    ds = AudiosetSrc(rcfg, "src_toy", True, label_map, True, echo=shown.append)
    assert ds.aclip_key == c["clip_key"] and len(ds) == 6 and ds.num_label == 5
    assert ds.sample_weights.dtype == np.float64 and ds.sample_weights.tolist() == c["sample_weights"]
    assert len(shown) == 1 and "\n" not in shown[0] and "speech 4" in shown[0]       # the label table: one plain line
    for i, want in enumerate(c["items"]):
        name, labels, clip_file = ds._process_item(i)
        assert name == want["name"] and clip_file == want["clip_file"].replace("ROOT", str(tmp_path), 1)
        assert labels == sorted(set(labels)) == [k for k, v in enumerate(want["label"]) if v]
        item = ds[i]
        assert set(item) == {"name", "labels", "pcm"} and np.array_equal(item["pcm"], clips[i]) and item["labels"] == labels
    for r in c["reads"]:
        fs = None if r["filter_set"] is None else set(r["filter_set"])
        d = AudiosetSrc(_cfg(tmp_path, prompt="the sound of", eval_samples=r["eval_samples"]).running, "src_toy", r["train"], label_map,
                        r["weighted"], filter_set=fs, echo=lambda s: None)
        assert [x["id"] for x in d.dataset] == r["ids"], r
        if r["weighted"]:
            assert d.sample_weights.tolist() == r["sample_weights"]
        else:
            assert not hasattr(d, "sample_weights")


# ------------------------------------------------------------------ 3. mixup draws and the tagging batch
def _tagging(tmp_path, n=12, **kw):
    from vipant_amd.data import build_audioset_label_map
    classes = ["/m/0a", "/m/0b", "/m/0c", "/m/0e", "/m/0h"]
    records = [{"id": f"t{i}", "dir": "bal" if i % 3 == 0 else "", "clip": ["wav"], "frame": "png",
                "labels": [classes[i % 5]] + ([classes[(i + 2) % 5]] if i % 2 else [])} for i in range(n)]
    records, clips = CF.make_audioset_dir(str(tmp_path), records=records, seconds=(0.05, 0.031, 0.042, 0.02), channels=(1, 2))
    cfg = _cfg(tmp_path, prompt="the sound of", **kw)
    label_map = build_audioset_label_map(str(tmp_path), "ontology,eval_segments", "the sound of", rcfg=cfg.running)
    return cfg, label_map, records, clips


def test_item_mixup_draws_follow_seed_index_and_epoch(tmp_path):
    from vipant_amd.data import AudiosetSrc
    from vipant_amd.data.classify import draw_item_mixup
    cfg, label_map, records, clips = _tagging(tmp_path, mixup_rate=0.5)
    ds = AudiosetSrc(cfg.running, "src_toy", True, label_map, False, seed=7)
    mixed, lams = 0, []
    for epoch in range(6):
        ds.set_epoch(epoch)
        for i in range(len(ds)):
            hit, partner, lam = draw_item_mixup(0.5, len(ds), torch.Generator().manual_seed(7 + 13 + i + 1000003 * epoch))
            item = ds[i]
            again = ds[i]
            assert set(item) == set(again) and item.get("lam") == again.get("lam")
            if hit and partner != i:
                assert set(item) == {"name", "labels", "pcm", "partner_pcm", "partner_labels", "lam"}
                assert np.array_equal(item["partner_pcm"], clips[partner]) and item["partner_labels"] == ds._process_item(partner)[1]
                assert item["lam"] == lam and np.float32(lam) == lam
                mixed += 1
                lams.append(lam)
            else:
                assert set(item) == {"name", "labels", "pcm"}
    assert 20 < mixed < 52 and 0.1 < min(lams) and max(lams) < 0.9 and 0.42 < np.mean(lams) < 0.58      # Beta(10, 10): sd 0.109
    # the same construction as the in-batch draw: b = 1 draws of KaldiFbank.draw_mixup give this lambda
    g1, g2 = torch.Generator().manual_seed(99), torch.Generator().manual_seed(99)
    _, _, lam = draw_item_mixup(1.0, 1, g1)
    u = torch.rand(1, generator=g2, dtype=torch.float64); torch.randint(0, 1, (1,), generator=g2)
    e = -torch.log1p(-torch.rand(1, 20, generator=g2, dtype=torch.float64))
    ga, gb = e[:, :10].sum(1), e[:, 10:].sum(1)
    assert lam == float((ga / (ga + gb)).to(torch.float32)) and 0.0 <= float(u) < 1.0
    # rate 1: everything is mixed but a clip that draws itself; evaluation and eval_norms draw nothing
    every = AudiosetSrc(_cfg(tmp_path, prompt="the sound of", mixup_rate=1.0).running, "src_toy", True, label_map, False, seed=7)
    selfs = [i for i in range(len(every)) if draw_item_mixup(1.0, len(every), every._generator(i))[1] == i]
    assert all(("lam" in every[i]) == (i not in selfs) for i in range(len(every)))
    one = AudiosetSrc(_cfg(tmp_path, prompt="the sound of", mixup_rate=1.0, eval_samples=1).running, "src_toy", False, label_map, False)
    assert len(one) == 1 and "lam" not in one[0]
    train_one = CF.make_audioset_dir(str(tmp_path), name="src_one", records=records[:1], seconds=(0.02,))
    alone = AudiosetSrc(_cfg(tmp_path, prompt="the sound of", mixup_rate=1.0).running, "src_one", True, label_map, False)
    assert "lam" not in alone[0] and train_one[0] == records[:1]                      # it can only draw itself
    for kw in (dict(train=False), dict(train=True, audio={"eval_norms": True})):
        d = AudiosetSrc(_cfg(tmp_path, prompt="the sound of", mixup_rate=1.0, audio=kw.get("audio", {"eval_norms": False})).running,
                        "src_toy", kw["train"], label_map, False, seed=7)
        assert all("lam" not in d[i] for i in range(len(d)))


def test_tagging_collator_layout(tmp_path):
    from vipant_amd.data import AudiosetSrc, PcmBatch, TaggingCollator, TaggingLabels
    cfg, label_map, records, clips = _tagging(tmp_path, mixup_rate=0.6)
    ds = AudiosetSrc(cfg.running, "src_toy", True, label_map, False, seed=3)
    items = [ds[i] for i in range(8)]
    mixed = [i for i, it in enumerate(items) if "lam" in it]
    assert 2 <= len(mixed) <= 7
    images, audios, text, labels, names = TaggingCollator(16000, 5)(items)
    b, p = 8, len(mixed)
    assert images.shape == (b, 1, 1, 1) and images.dtype == torch.float32 and text.shape == (b, 1) and text.dtype == torch.int64
    assert names == [r["id"] for r in records[:8]]
    assert isinstance(audios, PcmBatch) and audios.pcm.shape[0] == b + p == audios.nframes.shape[0] == audios.channels.shape[0]
    assert isinstance(labels, TaggingLabels) and labels.shape == (b, 5)
    assert labels.ids.dtype == labels.offsets.dtype == labels.mix_index.dtype == torch.int32 and labels.mix_lambda.dtype == torch.float32
    assert labels.offsets.shape == (b + p + 1,) and labels.mix_index.shape == (b,) == labels.mix_lambda.shape
    off = labels.offsets.tolist()
    assert off[0] == 0 and off[-1] == labels.ids.numel() and all(x <= y for x, y in zip(off, off[1:]))
    # partners after the batch, in the order of the clips that drew them; unmixed: -1 and lambda exactly 1
    assert labels.mix_index.tolist() == [b + mixed.index(i) if i in mixed else -1 for i in range(b)]
    for i, it in enumerate(items):
        assert labels.ids[off[i]:off[i + 1]].tolist() == it["labels"]
        assert int(audios.nframes[i]) == it["pcm"].shape[0] and np.array_equal(audios.pcm[i, :it["pcm"].size].numpy(), it["pcm"].reshape(-1))
        if i in mixed:
            r = b + mixed.index(i)
            assert labels.ids[off[r]:off[r + 1]].tolist() == it["partner_labels"] and float(labels.mix_lambda[i]) == it["lam"]
            assert int(audios.nframes[r]) == it["partner_pcm"].shape[0] and int(audios.channels[r]) == it["partner_pcm"].shape[1]
            assert np.array_equal(audios.pcm[r, :it["partner_pcm"].size].numpy(), it["partner_pcm"].reshape(-1))
        else:
            assert float(labels.mix_lambda[i]) == 1.0
    dense = labels.dense()
    assert dense.shape == (b + p, 5) and dense[1].tolist() == [0, 1, 0, 1, 0]        # t1: classes 1 and 3
    pinned = labels.to("cpu")
    assert isinstance(pinned, TaggingLabels) and torch.equal(pinned.ids, labels.ids) and pinned.num_label == 5
    # nothing mixed: b rows, every index -1
    plain = TaggingCollator(16000, 5)([{k: v for k, v in it.items() if k in ("name", "labels", "pcm")} for it in items])
    assert plain[1].pcm.shape[0] == b and plain[3].mix_index.tolist() == [-1] * b and plain[3].offsets.shape == (b + 1,)


def _flat(batch):
    lab = batch[3]
    return [batch[0], batch[1].pcm, batch[1].nframes, batch[1].channels, batch[2], lab.ids, lab.offsets, lab.mix_index, lab.mix_lambda], \
        list(batch[4])


def test_workers_do_not_change_a_batch_and_never_open_the_device(tmp_path):
    from vipant_amd.data import build_audioset_clf_dataloader, build_xfold_dataloader
    cfg0, label_map, records, clips = _tagging(tmp_path, mixup_rate=0.7)
    cfg2 = _cfg(tmp_path, workers=2, prompt="the sound of", mixup_rate=0.7)
    with _quiet():
        _, one = build_audioset_clf_dataloader(cfg0, "src_toy", label_map, shuffle=False, train=True, echo=lambda s: None)
        _, two = build_audioset_clf_dataloader(cfg2, "src_toy", label_map, shuffle=False, train=True, decode_audio=CF.checked_read_wav,
                                               echo=lambda s: None)
        assert two.num_workers == 2 and two.multiprocessing_context.get_start_method() == "spawn" and len(one) == 3
        a, b = list(one), list(two)
    assert len(a) == len(b) == 3 and any(int((x[3].mix_index >= 0).sum()) > 0 for x in a)
    for x, y in zip(a, b):
        (tx, nx), (ty, ny) = _flat(x), _flat(y)
        assert nx == ny and all(torch.equal(p, q) for p, q in zip(tx, ty))
    CF.make_esc50_dir(str(tmp_path))
    from vipant_amd.data import build_xfold_dataloader_list
    lists = build_xfold_dataloader_list(_cfg(tmp_path), echo=lambda s: None)[0]
    fold = lists[1][1].__defaults__[0] + lists[2][1].__defaults__[0]
    with _quiet():
        _, one = build_xfold_dataloader(_cfg(tmp_path, batch_size=3), fold, shuffle=False, train=False)
        _, two = build_xfold_dataloader(_cfg(tmp_path, workers=2, batch_size=3), fold, shuffle=False, train=False,
                                        decode_audio=CF.checked_read_wav)
        a, b = list(one), list(two)
    assert len(a) == len(b) == 2 and two.multiprocessing_context.get_start_method() == "spawn"
    for x, y in zip(a, b):
        assert torch.equal(x[0].pcm, y[0].pcm) and torch.equal(x[0].nframes, y[0].nframes) and torch.equal(x[1], y[1]) and x[2] == y[2]


def test_the_data_package_never_loads_the_binding():
    code = ("import sys; import vipant_amd.data, cvap.data; assert cvap.data.AudiosetSrc is vipant_amd.data.AudiosetSrc; "
            "assert cvap.data.build_xfold_dataloader_list is vipant_amd.data.build_xfold_dataloader_list; "
            "import torch; assert not torch.cuda.is_initialized(); "
            "assert 'vipant_amd._ffi' not in sys.modules and 'vipant_amd.ops' not in sys.modules, sorted(m for m in sys.modules if 'vipant' in m)")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


# ------------------------------------------------------------------ 4. the weighted sampler
def test_weighted_sampler_uses_the_recorded_weights_and_prefers_the_rare_class(tmp_path):
    from vipant_amd.data import AudiosetSrc, build_audioset_clf_dataloader, build_audioset_label_map
    c = GOLD["tagging"]["cases"][0]
    CF.make_audioset_dir(str(tmp_path))
    cfg = _cfg(tmp_path, prompt="the sound of", weighted_sampling=True, batch_size=2)
    label_map = build_audioset_label_map(str(tmp_path), "ontology,eval_segments", " the sound of ", rcfg=cfg.running)
    with _quiet():
        sampler, loader = build_audioset_clf_dataloader(cfg, "src_toy", label_map, shuffle=True, train=True, echo=lambda s: None)
        assert isinstance(sampler, torch.utils.data.WeightedRandomSampler) and loader.sampler is sampler
        assert sampler.weights.dtype == torch.float64 and sampler.weights.tolist() == c["sample_weights"]
        assert sampler.num_samples == 6 and sampler.replacement
        # evaluation, or the switch off: no weights
        s2, _ = build_audioset_clf_dataloader(cfg, "src_toy", label_map, shuffle=False, train=False, echo=lambda s: None)
        assert isinstance(s2, torch.utils.data.SequentialSampler)
        s3, l3 = build_audioset_clf_dataloader(_cfg(tmp_path, prompt="the sound of"), "src_toy", label_map, shuffle=True, train=True)
        assert isinstance(s3, torch.utils.data.RandomSampler) and not hasattr(l3.dataset, "sample_weights")
    # One class's weight dominant.  Inverse-frequency weights give a CLASS a total of 1000 n / (n + 1) < 1000 however many clips it
    # has, so single-label clips of one class never outweigh another class by much.  Here 2 clips carry the two rare labels {3, 4}
    # and 40 clips the common label {0}: a rare clip weighs 2 * 1000 / 3 = 666.7, a common one 1000 / 41 = 24.4, so a draw is a rare
    # clip with p = 1333.3 / (1333.3 + 975.6) = 0.577 (uniform sampling: 2 / 42 = 0.048).  Over 200 draws the count is
    # Binomial(200, 0.577): mean 115.5, sd 7.0 -- "more than half" has a margin of 2.2 sd; the seeded draw below gives 130.
    classes = ["/m/0a", "/m/0b", "/m/0c", "/m/0e", "/m/0h"]
    records = [{"id": f"w{i}", "dir": "", "clip": ["wav"], "frame": "png", "labels": [classes[0]] if i >= 2 else [classes[3], classes[4]]}
               for i in range(42)]
    CF.write_text(f"{tmp_path}/src_skew.csv", "".join(json.dumps(r) + "\n" for r in records))
    ds = AudiosetSrc(cfg.running, "src_skew", True, label_map, True, echo=lambda s: None)
    w = ds.sample_weights
    assert np.allclose(w[:2], 2000.0 / 3.0) and np.allclose(w[2:], 1000.0 / 41.0)
    p = w[:2].sum() / w.sum()
    assert 0.57 < p < 0.58
    sampler = torch.utils.data.WeightedRandomSampler(w, 200, replacement=True, generator=torch.Generator().manual_seed(5))
    picks = list(sampler)
    rare = sum(i < 2 for i in picks)
    print(f"rare clips drawn {rare} of 200 (p = {p:.3f})")
    assert len(picks) == 200 and rare > 100


# ------------------------------------------------------------------ 5. refusals
def test_refusals(tmp_path):
    from vipant_amd.data import AudiosetSrc, build_audioset_clf_dataloader, build_audioset_label_map, build_xfold_dataloader_list
    from vipant_amd.errors import VipantError
    CF.make_audioset_dir(str(tmp_path))
    label_map = build_audioset_label_map(str(tmp_path), "ontology,eval_segments", "", rcfg=_cfg(tmp_path).running)
    for name in ("audioset", "voxceleb2", "esc10", "mreserve"):
        with pytest.raises(VipantError, match="not built"):
            build_xfold_dataloader_list(_cfg(tmp_path, data_name=name))
    with pytest.raises(VipantError, match=r"meta/esc50\.csv is not a file\."):
        build_xfold_dataloader_list(_cfg(tmp_path, data_name="esc50"))
    with pytest.raises(VipantError, match=r"metadata/UrbanSound8K\.csv is not a file\."):
        build_xfold_dataloader_list(_cfg(tmp_path, data_name="UrbanSound8K"))
    for kw, msg in ((dict(clf=False), "clf=False"), (dict(imagine=True), "imagine"), (dict(cat_label=True), "cat_label"),
                    (dict(text_emb="emb"), "text_emb"), (dict(force_npz=True), "npz")):
        with pytest.raises(VipantError, match=msg):
            AudiosetSrc(_cfg(tmp_path, **kw).running, "src_toy", True, label_map, False)
        with pytest.raises(VipantError, match=msg):
            build_audioset_clf_dataloader(_cfg(tmp_path, **kw), "src_toy", label_map)
    with pytest.raises(VipantError, match="npz"):
        AudiosetSrc(_cfg(tmp_path).running, "npz_toy", True, label_map, False)
    with pytest.raises(VipantError, match=r"src_none\.csv is not a file\."):
        AudiosetSrc(_cfg(tmp_path).running, "src_none", True, label_map, False)
    with pytest.raises(VipantError, match="holds no record"):
        AudiosetSrc(_cfg(tmp_path).running, "src_toy", True, label_map, False, filter_set={"nobody"})
    with pytest.raises(VipantError, match="valid `ontology`"):
        build_audioset_label_map(str(tmp_path), "ontology,missing_segments", "", rcfg=_cfg(tmp_path).running)
    with pytest.raises(VipantError, match="valid `ontology`"):
        build_audioset_label_map(str(tmp_path), "ontology", "", rcfg=_cfg(tmp_path).running)
    with pytest.raises(VipantError, match=r"running\.bpe_path"):
        build_audioset_label_map(str(tmp_path), "ontology,eval_segments", "", rcfg=_cfg(tmp_path, bpe_path="").running)
    with pytest.raises(VipantError, match="running.sample_rate = 44100"):
        AudiosetSrc(_cfg(tmp_path, sample_rate=44100).running, "src_toy", True, label_map, False)[0]
