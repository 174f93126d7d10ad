"""Directories in the layout of the reference's classification datasets, generated into a temporary path with the writers of
tests/src_fixture.py from the toy inputs recorded in tests/golden/clf_dataset.json: an ESC-50 tree (`meta/esc50.csv`, clips in
`audio/`), an UrbanSound8K tree (`metadata/UrbanSound8K.csv`, clips in `audio/fold{k}/`) and an AudioSet tree (ontology, segments CSV,
filter files, `{name}.csv` index, clips under `{dir/}clip/`).  Shared by tests/test_clf_dataset_cpu.py and
tests/test_clf_src_trainer_gpu.py."""
import json
import os
import sys

import numpy as np

import src_fixture as SF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BPE = os.path.join(ROOT, "tests", "golden", "bpe_simple_vocab_16e6.head.txt.gz")
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "clf_dataset.json")))


def write_text(path, text):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(text)


def meta_rows(meta):
    return [line.split(",") for line in meta.strip().split("\n")[1:]]


def _clips(root, paths, seconds, channels, seed):
    """One clip per path, its level growing with its position (distinct features) -> {path below root: int16 [n, ch]}."""
    g = np.random.default_rng(seed)
    clips = {}
    for i, path in enumerate(paths):
        sec = seconds[i % len(seconds)]
        ch = channels[i % len(channels)]
        pcm = SF.noise_clip(g, int(round(sec * SF.SR)), ch, amp=700 + 450 * i)
        SF.write_wav(f"{root}/{path}", pcm)
        clips[path] = pcm
    return clips


def make_esc50_dir(root, ensemble=False, seconds=(0.5, 0.31, 0.42), channels=(1, 2), seed=21):
    """-> {`audio/{filename}`: clip}, in the order of the meta file."""
    write_text(f"{root}/meta/esc50.csv", GOLD["esc50"]["meta"])
    if ensemble:
        write_text(f"{root}/meta/ensemble.json", json.dumps(GOLD["esc50"]["ensemble"]))
    return _clips(root, [f"audio/{row[0]}" for row in meta_rows(GOLD["esc50"]["meta"])], seconds, channels, seed)


def make_us8k_dir(root, ensemble=False, seconds=(0.2, 0.25), channels=(1, 2), seed=22):
    write_text(f"{root}/metadata/UrbanSound8K.csv", GOLD["us8k"]["meta"])
    if ensemble:
        write_text(f"{root}/meta/ensemble.json", json.dumps(GOLD["us8k"]["ensemble"]))
    return _clips(root, [f"audio/fold{row[5]}/{row[0]}" for row in meta_rows(GOLD["us8k"]["meta"])], seconds, channels, seed)


def write_audioset_meta(root):
    a = GOLD["audioset"]
    write_text(f"{root}/ontology.json", json.dumps(a["ontology"]))
    write_text(f"{root}/eval_segments.csv", a["segments"])
    for fname, text in a["filter_files"].items():
        write_text(f"{root}/{fname}", text)


def make_audioset_dir(root, name="src_toy", clip_key="clip", records=None, seconds=(0.5, 0.31, 0.42, 0.5, 0.27, 1.0), channels=(1, 2),
                      seed=23):
    """The ontology / segments / filter files, the index `{name}.csv` (default: the recorded toy records) and its clips
    -> (records, clips in record order)."""
    write_audioset_meta(root)
    if records is None:
        records = next(c for c in GOLD["tagging"]["cases"] if c["clip_key"] == clip_key)["records"]
    write_text(f"{root}/{name}.csv", "".join(json.dumps(r) + "\n" for r in records))
    paths = [f"{r['dir'] + '/' if r['dir'] else ''}{clip_key}/{r['id']}.{r[clip_key][0]}" for r in records]
    clips = _clips(root, paths, seconds, channels, seed)
    return records, [clips[p] for p in paths]


def checked_read_wav(path):
    """read_wav for a loader worker that must never have opened the GPU or loaded the binding (module level: spawned workers import
    it by name)."""
    import torch
    from vipant_amd.data import read_wav
    if torch.cuda.is_initialized() or "vipant_amd._ffi" in sys.modules or "vipant_amd.ops" in sys.modules:
        raise RuntimeError("a loader process has the device or the binding open")
    return read_wav(path)
