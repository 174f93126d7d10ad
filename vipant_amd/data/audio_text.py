"""The caption datasets of the AT trainer (`monitor=VALMonitor running.data_root=DIR`): AudioCaps in the raw-file layout
(cvap/data/audiocaps.py:33-232 `AudioCapDatasetSrc`, what VALMonitor reads for `data_name=audiocaps*`) and the audio-text lists
(cvap/data/audio_text.py: `AudioTextDatasetSrc`, `build_clotho_data_list`, `build_audiocaps_data_list`, the builder :233-245).

Host only, like the rest of the package: a worker decodes the WAV (and, under `running.imagine`, the frame) and picks the caption; the
captions were tokenised once, when the index was read (vipant_amd/tokenizer.py).  Waveform, log-mel, augmentation and image transform
run on the device in the trainer's `make_batch`, so an item is {"pcm": int16 [n, ch], "name": id, "text": ids or a list of ids} plus
"frame" / "embed" when an image is shown.  Index, path, frame and caption rules are the reference's; the deviations are those of
image_audio.py (one sample rate, per-item generator, seeded `train_samples` subset), and `clf=True` -- the in-dataset mixup branch
`_audio2numpy_clf` -- is refused: tagging has its own trainer.
"""
from __future__ import annotations

import csv
import itertools
import json
import os

import numpy as np
import torch
import torch.utils.data as data

from ..errors import VipantError
from .decode import read_frame, read_wav
from .image_audio import ImageAudioSrc, _collate_frames, _collate_pcm


def _tokenizer(rcfg, tokenizer=None):
    """-> (the tokenizer of this run, `tokenize`); imported here, so that the image-audio datasets do not need the `regex` module."""
    from ..tokenizer import load_tokenizer, tokenize
    return (tokenizer if tokenizer is not None else load_tokenizer(rcfg)), tokenize


def _refuse_clf(rcfg):
    if rcfg.get("clf", False):
        raise VipantError("running.clf=True: the caption datasets do not mix clips inside the dataset (`_audio2numpy_clf`); "
                          "tagging with mixup is monitor=ASMonitor")


class AudioCapSrc(ImageAudioSrc):
    """`__getitem__` decodes one clip of `{data_root}/{data_name}.csv` and hands over its caption(s): training one caption, drawn
    (under `running.rnd_cap` from the captions of a record drawn first); evaluation all of them.  Under `running.imagine` the item
    also holds the frame, or its embedding when `running.frame_emb` is set, by ImageAudioSrc's rules.  Draws of an item, from its
    own generator and in the reference's order: frame index, `rnd_cap` record, caption index."""

    def __init__(self, rcfg, data_name, train, decode_audio=None, decode_frame=None, seed=0, tokenizer=None):
        _refuse_clf(rcfg)
        super().__init__(rcfg, data_name, train, decode_audio=decode_audio, decode_frame=decode_frame, seed=seed)
        tokenizer, tokenize = _tokenizer(rcfg, tokenizer)
        for record in self.dataset:             # no prompt in front of an AudioCaps caption (audiocaps.py:46-48)
            record["captions_bpe"] = tokenize(record["captions"], as_list=True, tokenizer=tokenizer)
        self.imagine = bool(rcfg.get("imagine", True))
        self.rnd_cap = bool(getattr(rcfg, "rnd_cap", False))        # random AL fine-tuning baseline (audiocaps.py:64)

    def _caption_item(self, index, generator=None):
        """audiocaps.py:81-115 -> (name, text, clip file, frame file, frame embedding file)."""
        generator = generator if generator is not None else self._generator(index)
        name, clip_file, frame_file, embed_file = self._process_item(index, generator, frames=self.imagine)
        captions = self.dataset[index]["captions_bpe"]
        if self.train:
            if self.rnd_cap:
                captions = self.dataset[int(torch.randint(self.length, (1,), generator=generator))]["captions_bpe"]
            text = captions[int(torch.randint(len(captions), (1,), generator=generator))]
        else:
            text = captions
        return name, text, clip_file, frame_file, embed_file

    def __getitem__(self, index):
        g = self._generator(index)
        name, text, clip_file, frame_file, embed_file = self._caption_item(index, g)
        item = {"name": name, "text": text}
        if embed_file is not None:
            item["embed"] = self._embed(embed_file, g)
        elif frame_file is not None:
            item["frame"] = self._frame(frame_file, g)
        item["pcm"] = self._pcm(clip_file)
        return item


class AudioTextSrc(ImageAudioSrc):
    """audio_text.py:23-103 over a list of records {"id", "dir", "clip" | "aclip": [ext or the file name], "label_int_bpe"}: a clip
    whose listed name is its id is read as `{root}/{dir/}{id}` (Clotho), any other as `{root}/{dir/}{akey}/{id}.{ext}`.  No image."""

    def __init__(self, rcfg, data_list, train, decode_audio=None, seed=0):
        _refuse_clf(rcfg)
        self.dataset = []
        for iline, record in enumerate(data_list):
            self.dataset.append(record)
            if not train and iline + 1 == rcfg.eval_samples:
                break
        if not self.dataset:
            raise VipantError("the audio-text list holds no record.")
        self.seed, self.epoch = int(seed), 0
        self.aclip_key = "clip" if "clip" in self.dataset[0] else "aclip"
        self.length, self.train = len(self.dataset), bool(train)
        self.data_root = str(rcfg.data_root)
        self.sample_rate = int(rcfg.get("sample_rate", 16000))
        self.decode_audio = decode_audio if decode_audio is not None else read_wav
        self.decode_frame, self.frame_emb, self.imagine = read_frame, None, False

    def _caption_item(self, index, generator=None):
        record = self.dataset[index]
        name, sub, aclip = record["id"], record["dir"], record[self.aclip_key][0]
        sub = "" if len(sub) == 0 else f"{sub}/"
        aclip = aclip if aclip == name else f"{self.aclip_key}/{name}.{aclip}"
        text = record["label_int_bpe"]
        if self.train:
            generator = generator if generator is not None else self._generator(index)
            text = text[int(torch.randint(len(text), (1,), generator=generator))]
        return name, text, f"{self.data_root}/{sub}{aclip}", None, None

    def __getitem__(self, index):
        name, text, clip_file, _, _ = self._caption_item(index)
        return {"name": name, "text": text, "pcm": self._pcm(clip_file)}


def collate_text(text_list):
    """Rows of token ids -- one per item when training, a list of rows per item at evaluation (chained, an item's rows contiguous)
    -- -> int64 [n, L], L the longest row, zero filled: `zip_longest(fillvalue=0)` of audioset_clf.py:138-147."""
    first = text_list[0][0] if len(text_list[0]) > 0 else None
    if isinstance(first, list):
        text_list = list(itertools.chain.from_iterable(text_list))
    elif not isinstance(first, int):
        raise ValueError(f"unrecognized `{type(first)}`")
    text = torch.zeros(len(text_list), max(len(row) for row in text_list), dtype=torch.int64)
    for i, row in enumerate(text_list):
        text[i, :len(row)] = torch.tensor(row, dtype=torch.int64)
    return text


class CaptionCollator:
    """Items -> the trainers' five-slot tuple (images, audios, text, labels, names): images a FrameBatch, fp32 [b, E] embeddings, or
    the reference's dummy ones [b, 1, 1, 1] when nothing is imagined; audios a PcmBatch; text int64 [n, L] (`collate_text`; n = b
    when training, the sum of the caption counts at evaluation); labels int64 [b] zeros.  Everything is on the CPU."""

    def __init__(self, sample_rate=16000):
        self.sample_rate = int(sample_rate)

    def __call__(self, items):
        b = len(items)
        if all("embed" in it for it in items):
            images = torch.from_numpy(np.stack([np.asarray(it["embed"], dtype=np.float32) for it in items]))
        elif all("frame" in it for it in items):
            images = _collate_frames(items)
        elif not any("embed" in it or "frame" in it for it in items):
            images = torch.ones(b, 1, 1, 1)
        else:
            raise VipantError("a batch mixes frames and frame embeddings (records with a single frame name have no embedding file)")
        return (images, _collate_pcm(items, self.sample_rate), collate_text([it["text"] for it in items]),
                torch.zeros(b, dtype=torch.int64), [it["name"] for it in items])


def _prompt(rcfg):
    prompt = str(rcfg.get("prompt", "") or "").strip()
    return "" if len(prompt) == 0 else f"{prompt} "


def build_clotho_data_list(rcfg, data_name, tokenizer=None):
    """audio_text.py:169-194: `{data_root}/{data_name}.csv` with the columns file_name, caption_1 .. caption_5 -> records whose clip
    is the file itself, inside the fold directory (the suffix of the data name: development | validation | evaluation)."""
    fold = data_name.rsplit("_", 1)[-1]
    data_path = f"{rcfg.data_root}/{data_name}.csv"
    if not os.path.isfile(data_path):
        raise VipantError(f"{data_path} is not a file.")
    tokenizer, tokenize = _tokenizer(rcfg, tokenizer)
    prompt = _prompt(rcfg)
    dataset = []
    with open(data_path, "r") as fr:
        for row in csv.DictReader(fr):
            filename = row["file_name"]
            captions = [prompt + row[f"caption_{icap}"] for icap in range(1, 6)]
            dataset.append({"id": filename, "dir": fold, "aclip": [filename],
                            "label_int_bpe": tokenize(captions, as_list=True, tokenizer=tokenizer), "label_int_w2v": [],
                            "label_str": captions})
    return dataset


def build_audiocaps_data_list(rcfg, data_name, tokenizer=None):
    """audio_text.py:196-215: the AudioCaps index as an audio-text list, `running.prompt` in front of every caption."""
    data_path = f"{rcfg.data_root}/{data_name}.csv"
    if not os.path.isfile(data_path):
        raise VipantError(f"{data_path} is not a file.")
    tokenizer, tokenize = _tokenizer(rcfg, tokenizer)
    prompt = _prompt(rcfg)
    dataset = []
    with open(data_path, "r") as fr:
        for line in fr:
            record = json.loads(line)
            captions = [prompt + caption for caption in record["captions"]]
            record["label_int_w2v"] = []
            record["label_int_bpe"] = tokenize(captions, as_list=True, tokenizer=tokenizer)
            record["label_str"] = captions
            dataset.append(record)
    return dataset


def build_audio_text_dataloader(cfg, data_name, shuffle=True, train=True, decode_audio=None, decode_frame=None):
    """-> (sampler, loader): `audiocaps*` reads AudioCapSrc (audioset_hub.py:118-119, VALMonitor's reader), `clotho*` AudioTextSrc
    over the Clotho lists of a comma-separated `data_name` (audio_text.py:217-223).  Sampler, per-rank batch, spawned workers and
    pinned memory as in `build_image_audio_dataloader`."""
    rcfg = cfg.running
    data_name = str(data_name)
    if data_name.startswith("audiocaps"):
        dataset = AudioCapSrc(rcfg, data_name, train, decode_audio=decode_audio, decode_frame=decode_frame, seed=int(cfg.seed))
    elif data_name.startswith("clotho"):
        tokenizer, _ = _tokenizer(rcfg)
        data_list = []
        for name in data_name.split(","):
            data_list.extend(build_clotho_data_list(rcfg, name, tokenizer=tokenizer))
        dataset = AudioTextSrc(rcfg, data_list, train, decode_audio=decode_audio, seed=int(cfg.seed))
    else:
        raise ValueError(f"unrecognized dataset `{data_name}`.")
    replicas = torch.distributed.is_available() and torch.distributed.is_initialized()
    if replicas:
        sampler = data.distributed.DistributedSampler(dataset, shuffle=shuffle, drop_last=True)
    else:
        sampler = data.RandomSampler(dataset) if shuffle else data.SequentialSampler(dataset)
    workers = int(cfg.get("num_proc", 0) or 0)
    loader = data.DataLoader(
        dataset, batch_size=int(rcfg.batch_size), collate_fn=CaptionCollator(dataset.sample_rate), num_workers=workers,
        pin_memory=True, sampler=sampler, drop_last=bool(replicas),
        # spawn: a forked worker would inherit the parent's open device
        multiprocessing_context=("spawn" if workers > 0 else None))
    return sampler, loader
