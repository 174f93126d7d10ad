"""The classification datasets that read raw files: the x-fold sets of the supervised trainer (cvap/data/esc50.py:27-111 and :194-324,
`monitor=ESCMonitor`: ESC-50 and UrbanSound8K) and AudioSet tagging (cvap/data/audioset_cls.py:193-466 `AudiosetSrc` on its `clf`
path, cvap/data/audioset_hub.py:32-106 label map and filter set, cvap/data/audioset_clf.py:154-194 the builder;
`monitor=ASMonitor`).

Host only, like the rest of the package: a worker decodes WAV containers to int16 and nothing else; nothing here imports the HIP
binding, calls torch.cuda or returns a device tensor.  Waveform, mixup, log-mel, norms and masks run on the device in the trainer's
`make_batch`.  So an x-fold item is {"pcm": int16 [n, ch], "label_int", "label_str"} and a tagging item {"pcm", "labels": the sorted
class indices of the clip, "name"} -- the multi-hot rows of 527 the reference builds per item are formed on the device from the
ragged lists (vipant_multihot_mix).

Mixup follows the reference in WHERE the partner comes from: it is drawn from the whole dataset in the worker (audioset_cls.py:381-400),
not from the batch.  A mixed item carries the partner's decoded clip, its labels and lambda; the collator appends the partner clips
behind the batch and the log-mel launch reads them as rows that produce no output (vipant_fbank_mix_src).  The mixing arithmetic
itself runs on the device.  Deviations: the draws come from the item's own generator (seed, index, epoch)
instead of the worker's `random` / numpy state, so a batch does not depend on the number of workers -- u < mixup_rate, the partner
uniform over the dataset, lambda ~ Beta(10, 10) by KaldiFbank.draw_mixup's Gamma construction; a clip that draws itself stays
unmixed; a clip whose sample rate differs from `running.sample_rate` is refused; the label table of the weighted sampler is one
plain line.
"""
from __future__ import annotations

import copy
import itertools
import json
import os
import re

import numpy as np
import torch
import torch.utils.data as data

from ..errors import VipantError
from .audio_text import _tokenizer
from .decode import read_wav
from .image_audio import ImageAudioSrc, _collate_pcm


# ------------------------------------------------------------------------------------------------ x-fold: ESC-50 / UrbanSound8K
class XFoldSrc(ImageAudioSrc):
    """esc50.py:27-111 over a list of records {"aclip": path below the data root, "label_int", "label_str"}: `__getitem__` decodes
    the clip -> {"pcm": int16 [n, ch], "label_int", "label_str"}.  `eval_samples` cuts an evaluation list as the reference does."""

    def __init__(self, rcfg, data_list, train, decode_audio=None, seed=0):
        self.dataset = []
        for iline, record in enumerate(data_list):
            self.dataset.append(record)
            if not train and iline + 1 == rcfg.eval_samples:
                break
        if not self.dataset:
            raise VipantError("the x-fold list holds no record.")
        self.seed, self.epoch = int(seed), 0
        self.length, self.train = len(self.dataset), bool(train)
        self.data_root = str(rcfg.data_root)
        self.sample_rate = int(rcfg.get("sample_rate", 16000))
        self.decode_audio = decode_audio if decode_audio is not None else read_wav

    def __getitem__(self, index):
        record = self.dataset[index]
        return {"pcm": self._pcm(f"{self.data_root}/{record['aclip']}"), "label_int": record["label_int"],
                "label_str": record["label_str"]}


class XFoldCollator:
    """Items -> (PcmBatch, labels int64 [b], names: the label strings), the three slots of esc50.py:113-127.  On the CPU."""

    def __init__(self, sample_rate=16000):
        self.sample_rate = int(sample_rate)

    def __call__(self, items):
        return (_collate_pcm(items, self.sample_rate), torch.tensor([int(it["label_int"]) for it in items], dtype=torch.int64),
                [it["label_str"] for it in items])


def _loader(cfg, dataset, collator, shuffle, sampler=None):
    """Sampler, per-rank batch, spawned workers and pinned memory as in `build_image_audio_dataloader`."""
    replicas = torch.distributed.is_available() and torch.distributed.is_initialized()
    if replicas:
        sampler = data.distributed.DistributedSampler(dataset, shuffle=shuffle, drop_last=True)
    elif sampler is None:
        sampler = data.RandomSampler(dataset) if shuffle else data.SequentialSampler(dataset)
    workers = int(cfg.get("num_proc", 0) or 0)
    loader = data.DataLoader(
        dataset, batch_size=int(cfg.running.batch_size), collate_fn=collator, num_workers=workers, pin_memory=True,
        sampler=sampler, drop_last=bool(replicas),
        # spawn: a forked worker would inherit the parent's open device
        multiprocessing_context=("spawn" if workers > 0 else None))
    return sampler, loader


def build_xfold_dataloader(cfg, data_list, shuffle=True, train=True, decode_audio=None):
    """esc50.py:194-222 -> (sampler, loader)."""
    dataset = XFoldSrc(cfg.running, data_list, train, decode_audio=decode_audio, seed=int(cfg.seed))
    return _loader(cfg, dataset, XFoldCollator(dataset.sample_rate), shuffle)


def _read_meta(data_path):
    if not os.path.isfile(data_path):
        raise VipantError(f"{data_path} is not a file.")
    return np.atleast_2d(np.loadtxt(data_path, delimiter=",", dtype="str", skiprows=1))


def _fold_loaders(cfg, folds, decode_audio):
    """Per held-out fold a lazy (train loader over the other folds, eval loader over the fold) pair (esc50.py:242-255)."""
    loader_tuple = tuple()
    nfold = len(folds)
    for i in range(nfold):
        train_list = []
        for j in range(nfold):
            if j == i:
                continue
            train_list.extend(copy.deepcopy(folds[j]))
        eval_list = copy.deepcopy(folds[i])
        loader_tuple += ((
            lambda data_list=train_list: build_xfold_dataloader(cfg, data_list, decode_audio=decode_audio),
            lambda data_list=eval_list: build_xfold_dataloader(cfg, data_list, shuffle=False, train=False, decode_audio=decode_audio)
        ),)
    return loader_tuple


def _pad_rows(rows):
    """`np.array(list(zip_longest(*rows, fillvalue=0))).T`: token rows zero-padded to a common width (row-major: the trainer turns it
    into the text tower's input as it is)."""
    return np.ascontiguousarray(np.array(list(itertools.zip_longest(*rows, fillvalue=0))).T)


def _plain_prompts(rcfg, lid2str):
    prompt = str(rcfg.get("prompt", "") or "").strip()
    prompt = "" if prompt == "" else prompt + " "
    return [prompt + lid2str[i].replace("_", " ") for i in range(len(lid2str))]


def build_dataloader_list_esc50(cfg, decode_audio=None, tokenizer=None, echo=None):
    """esc50.py:224-276: `meta/{data_name}.csv` (filename, fold, target, category, ...), 5 folds, clips in `audio/`."""
    rcfg = cfg.running
    meta = _read_meta(f"{rcfg.data_root}/meta/{rcfg.data_name}.csv")
    folds = [[] for _ in range(5)]
    lid2str = dict()
    for row in meta:
        filename, fold, target, category = row[:4]
        folds[int(fold) - 1].append({"aclip": f"audio/{filename}", "label_int": int(target), "label_str": str(category)})
        lid2str[int(target)] = str(category)
    loader_tuple = _fold_loaders(cfg, folds, decode_audio)
    label_path = f"{rcfg.data_root}/meta/{rcfg.get('prompt', '')}.json"
    if not os.path.isfile(label_path):
        lid2int = _plain_prompts(rcfg, lid2str)
        label_map = {i: i for i in range(len(lid2str))}
    else:                                                       # the prompt ensemble: the first 4 texts of every class
        topk = 4
        with open(label_path, "r") as fr:
            label_map = json.load(fr)
        text_list = [label_map[lid2str[i].replace("_", " ")][:topk] for i in range(len(lid2str))]
        lid2int = list(itertools.chain.from_iterable(text_list))
        lid2int = [re.sub("^a photo of", "the sound of", text) for text in lid2int]
        if len(lid2int) != len(text_list) * topk:
            raise VipantError(f"unbalanced label mapping: {len(text_list)}x{topk} -> {len(lid2int)}")
        label_map = {i: i // topk for i in range(len(lid2str) * topk)}
    (echo or print)(f"{lid2int}")
    tokenizer, tokenize = _tokenizer(rcfg, tokenizer)
    lid2int = _pad_rows(tokenize(lid2int, as_list=True, tokenizer=tokenizer))
    return loader_tuple, lid2str, lid2int, label_map


def build_dataloader_list_us8k(cfg, decode_audio=None, tokenizer=None, echo=None):
    """esc50.py:278-324: `metadata/{data_name}.csv` (slice_file_name, ..., fold, classID, class), 10 folds, clips in
    `audio/fold{k}/`.  No label map, as in the reference; with `meta/{prompt}.json` present the prompts are the bare names."""
    rcfg = cfg.running
    meta = _read_meta(f"{rcfg.data_root}/metadata/{rcfg.data_name}.csv")
    folds = [[] for _ in range(10)]
    lid2str = dict()
    for row in meta:
        filename, fold, target, category = row[0], row[5], row[6], row[7]
        folds[int(fold) - 1].append({"aclip": f"audio/fold{fold}/{filename}", "label_int": int(target), "label_str": str(category)})
        lid2str[int(target)] = str(category)
    loader_tuple = _fold_loaders(cfg, folds, decode_audio)
    label_path = f"{rcfg.data_root}/meta/{rcfg.get('prompt', '')}.json"
    if not os.path.isfile(label_path):
        lid2int = _plain_prompts(rcfg, lid2str)
    else:
        lid2int = [lid2str[i].replace("_", " ") for i in range(len(lid2str))]
    (echo or print)(f"{lid2int}")
    tokenizer, tokenize = _tokenizer(rcfg, tokenizer)
    lid2int = _pad_rows(tokenize(lid2int, as_list=True, tokenizer=tokenizer))
    return loader_tuple, lid2str, lid2int, None


def build_xfold_dataloader_list(cfg, decode_audio=None, tokenizer=None, echo=None):
    """esc50.py:448-458 -> (loader_list, lid2str, lid2int, label_map), what `ESCMonitor.build_data` takes through `loader_list=`."""
    name = str(cfg.running.data_name)
    if name == "esc50":
        return build_dataloader_list_esc50(cfg, decode_audio=decode_audio, tokenizer=tokenizer, echo=echo)
    if name == "UrbanSound8K":
        return build_dataloader_list_us8k(cfg, decode_audio=decode_audio, tokenizer=tokenizer, echo=echo)
    raise VipantError(f"x-fold dataset `{name}`: not built (the x-fold sets that are: esc50, UrbanSound8K)")


# ------------------------------------------------------------------------------------------------ AudioSet: label map and filter set
def build_filter_set(data_root, filter_set):
    """audioset_hub.py:32-58: `name,topk` -> the set of clip ids training may use, or None on ANY failure (no filter configured
    included).  `name` ending in csv: one id per line; ending in k: a JSON object label -> ids; anything else: one JSON object per
    line, id -> [[neighbour id, score], ...], of which the first `topk` neighbours and the id itself are taken."""
    try:
        name, topk = filter_set.split(",")
        filter_file = f"{data_root}/{name}"
        if filter_file[-3:] == "csv":
            samples = set()
            with open(filter_file, "r") as fr:
                for line in fr:
                    samples.add(line.strip())
        elif filter_file[-1] == "k":
            with open(filter_file, "r") as fr:
                samples_per_label = json.load(fr)
            samples = set()
            for k, v in samples_per_label.items():
                samples.update(v)
        else:
            topk = int(topk)
            samples = set()
            with open(filter_file, "r") as fr:
                for line in fr:
                    line = json.loads(line)
                    k, v = list(line.items())[0]
                    samples.update(set([name for name, _ in v[:topk]] + [k]))
    except Exception:
        samples = None
    return samples


def collect_ytid(csv_root, csv_list):
    """audioset_hub.py:60-74: the segments CSVs (three header lines, then `ytid, start, end, "a,b,c"`) -> (ids, id -> rows)."""
    ids = dict()
    for fname in csv_list:
        with open(f"{csv_root}/{fname}.csv", "r") as fr:
            for _ in range(3):
                next(fr)
            for row in fr:
                row = row.split(", ")
                ids.setdefault(row[0].strip(), []).append((row[1].strip(), row[2].strip(), row[3].strip('" \n').split(",")))
    return list(ids.keys()), ids


def build_audioset_label_map(data_root, label_map="ontology,eval_segments", prompt="", tokenizer=None, rcfg=None):
    """audioset_hub.py:76-106: the ontology restricted to the classes seen in the segments CSVs (the first row of every clip) ->
    {class id: (index, prompt + lower-cased name, tokens)}.  The tokenizer: the one given, else the run's (`rcfg`), else the
    module's current one."""
    file_list = str(label_map).split(",")
    ontology, label_files = file_list[0], file_list[1:]
    label_path = f"{data_root}/{ontology}.json"
    if not label_files or not os.path.isfile(label_path) or not os.path.isfile(f"{data_root}/{label_files[0]}.csv"):
        raise VipantError("please specify a valid `ontology` file (ontology) and `eval` file (eval_segments): "
                          f"running.label_map=`{label_map}` under `{data_root}`")
    with open(label_path, "r") as fr:
        ontology = json.load(fr)
    prompt = "" if prompt.strip() == "" else prompt.strip() + " "
    category_list = [(item["id"], prompt + item["name"].lower()) for item in ontology]
    if tokenizer is None and rcfg is not None:
        tokenizer, _ = _tokenizer(rcfg)
    from ..tokenizer import tokenize
    label_int = tokenize([item[1] for item in category_list], as_list=True, tokenizer=tokenizer)
    category_list = [item + (label_int[i],) for i, item in enumerate(category_list)]
    _, ytid_dict = collect_ytid(data_root, label_files)
    label_set = set(itertools.chain.from_iterable(v[0][2] for _, v in ytid_dict.items()))
    category_list = [item for item in category_list if item[0] in label_set]
    return {category_list[i][0]: (i,) + category_list[i][1:] for i in range(len(category_list))}


# ------------------------------------------------------------------------------------------------ AudioSet tagging
def draw_item_mixup(rate, length, generator):
    """The mixup draws of ONE item, in a fixed order and number whatever fires: u against `rate`, the partner uniform in
    [0, length), lambda ~ Beta(10, 10) as the ratio of two Gamma(10) sums of exponentials (KaldiFbank.draw_mixup's construction)
    -> (mixed, partner, lambda as float32)."""
    u = float(torch.rand(1, generator=generator, dtype=torch.float64))
    partner = int(torch.randint(0, max(int(length), 1), (1,), generator=generator))
    e = -torch.log1p(-torch.rand(20, generator=generator, dtype=torch.float64))
    ga, gb = e[:10].sum(), e[10:].sum()
    return u < float(rate), partner, float((ga / (ga + gb)).to(torch.float32))


class AudiosetSrc(ImageAudioSrc):
    """audioset_cls.py:193-466 on its classification path (`running.clf`): `{data_root}/{data_name}.csv`, one JSON record per
    line with `labels`.  `__getitem__` -> {"pcm": int16 [n, ch], "labels": sorted unique class indices, "name": id}, and for a
    training item whose generator draws u < `running.mixup_rate` (with `running.audio.eval_norms` off) also {"partner_pcm",
    "partner_labels", "lam"}.  `weighted=True` computes `sample_weights` float64 [length] (:216-231)."""

    def __init__(self, rcfg, data_name, train, label_map, weighted, filter_set=None, decode_audio=None, seed=0, echo=None):
        data_name = str(data_name)
        if data_name.startswith("npz") or rcfg.get("force_npz", False):
            raise VipantError("npz datasets (`npz*` names, running.force_npz): not built")
        if not rcfg.get("clf", True):
            raise VipantError("running.clf=False: the AudioSet dataset with text (one label's prompt per clip) is not built; "
                              "the tagging dataset is the clf path")
        if rcfg.get("imagine", False):
            raise VipantError("running.imagine=True: the tagging dataset shows no frames (imagine-and-classify from files is not built)")
        if rcfg.get("cat_label", False):
            raise VipantError("running.cat_label=True: concatenated label captions belong to the text path, which is not built")
        if rcfg.get("text_emb", None) is not None:
            raise VipantError("running.text_emb: pre-computed text embeddings belong to the text path, which is not built")
        data_path = f"{rcfg.data_root}/{data_name}.csv"
        if not os.path.isfile(data_path):
            raise VipantError(f"{data_path} is not a file.")
        self.label_map = label_map
        self.num_label = len(label_map)
        label_counts = np.zeros(self.num_label)
        self.dataset = []
        with open(data_path, "r") as fr:
            for iline, line in enumerate(fr):
                record = json.loads(line)
                if filter_set is not None and record["id"] not in filter_set:
                    continue                                    # let us skip this sample
                self.dataset.append(record)
                if not train and iline + 1 == rcfg.eval_samples:
                    break
                if weighted:                                    # save label distribution
                    for category in record["labels"]:
                        label_counts[self.label_map[category][0]] += 1
        if not self.dataset:
            raise VipantError(f"{data_path} holds no record (after the filter set).")
        self.length = len(self.dataset)
        if weighted:                                            # compute sample weight
            prompt = str(rcfg.get("prompt", "") or "")
            lid2label = {v[0]: re.sub(f"^{prompt}", "", v[1]).strip() for _, v in label_map.items()}
            (echo or print)("label distribution: " + " | ".join(f"{lid2label[i]} {int(label_counts[i])}" for i in range(self.num_label)))
            self.sample_weights = np.zeros(self.length)
            label_counts = 1000.0 / (label_counts + 1.)
            for i, record in enumerate(self.dataset):
                for category in record["labels"]:
                    self.sample_weights[i] += label_counts[self.label_map[category][0]]
        self.aclip_key = "clip" if "clip" in self.dataset[0] else "aclip"
        self.seed, self.epoch, self.train = int(seed), 0, bool(train)
        self.data_root = str(rcfg.data_root)
        self.sample_rate = int(rcfg.get("sample_rate", 16000))
        self.decode_audio = decode_audio if decode_audio is not None else read_wav
        acfg = rcfg.get("audio", None) or {}
        self.mixup_rate = float(rcfg.get("mixup_rate", 0.0) or 0.0) if (self.train and not acfg.get("eval_norms", False)) else 0.0

    def _process_item(self, index):
        """audioset_cls.py:269-310, clf branch -> (name, sorted unique class indices, clip file).  The reference's multi-hot row is
        `[1 if i in set(labels) else 0 for i in range(num_label)]`."""
        record = self.dataset[index]
        akey, sub_dir, name = self.aclip_key, record["dir"], record["id"]
        sub_dir = "" if len(sub_dir) == 0 else f"{sub_dir}/"
        aclip_file = f"{self.data_root}/{sub_dir}{akey}/{name}.{record[akey][0]}"
        labels = sorted(set(self.label_map[category][0] for category in record["labels"]))
        return name, labels, aclip_file

    def __getitem__(self, index):
        name, labels, aclip_file = self._process_item(index)
        item = {"name": name, "labels": labels, "pcm": self._pcm(aclip_file)}
        if self.mixup_rate > 0:
            mixed, partner, lam = draw_item_mixup(self.mixup_rate, self.length, self._generator(index))
            if mixed and partner != int(index):                 # a clip that draws itself stays unmixed
                _, partner_labels, partner_file = self._process_item(partner)
                item.update({"partner_pcm": self._pcm(partner_file), "partner_labels": partner_labels, "lam": lam})
        return item


class TaggingLabels:
    """The label slot of a tagging batch: the ragged class lists of the b clips and, behind them, of the p partner clips -- ids int32
    [total], offsets int32 [b + p + 1] --, mix_index int32 [b] (-1, or the row b + k of the clip's partner), mix_lambda fp32 [b] (1
    where not mixed) and the number of classes.  `dense()` is the host's multi-hot [b + p, C] (tests, reports)."""

    def __init__(self, ids, offsets, mix_index, mix_lambda, num_label):
        self.ids, self.offsets, self.mix_index, self.mix_lambda, self.num_label = ids, offsets, mix_index, mix_lambda, int(num_label)

    def to(self, device, non_blocking=False):
        return TaggingLabels(*(t.to(device, non_blocking=non_blocking) for t in (self.ids, self.offsets, self.mix_index, self.mix_lambda)),
                             self.num_label)

    def pin_memory(self):
        return TaggingLabels(*(t.pin_memory() for t in (self.ids, self.offsets, self.mix_index, self.mix_lambda)), self.num_label)

    @property
    def shape(self):
        return (self.mix_index.shape[0], self.num_label)

    def dense(self):
        off = self.offsets.tolist()
        y = torch.zeros(len(off) - 1, self.num_label)
        for r in range(len(off) - 1):
            for c in self.ids[off[r]:off[r + 1]].tolist():
                y[r, c] = 1.0
        return y


class TaggingCollator:
    """Items of AudiosetSrc -> the reference's five slots (audioset_clf.py:122-152): images fp32 ones [b, 1, 1, 1] (nothing is
    imagined), audios a PcmBatch of b + p rows -- the p partner clips behind the batch, in the order of the clips that drew them --,
    text int64 zeros [b, 1], labels a TaggingLabels over the same b + p rows, names.  Everything is on the CPU."""

    def __init__(self, sample_rate=16000, num_label=527):
        self.sample_rate, self.num_label = int(sample_rate), int(num_label)

    def __call__(self, items):
        b = len(items)
        rows = [{"pcm": it["pcm"]} for it in items]
        lists = [list(it["labels"]) for it in items]
        mix_index = torch.full((b,), -1, dtype=torch.int32)
        mix_lambda = torch.ones(b, dtype=torch.float32)
        for i, it in enumerate(items):
            if "partner_pcm" in it:
                mix_index[i], mix_lambda[i] = len(rows), float(it["lam"])
                rows.append({"pcm": it["partner_pcm"]})
                lists.append(list(it["partner_labels"]))
        offsets = torch.tensor([0] + list(itertools.accumulate(len(row) for row in lists)), dtype=torch.int32)
        ids = torch.tensor(list(itertools.chain.from_iterable(lists)), dtype=torch.int32)
        labels = TaggingLabels(ids, offsets, mix_index, mix_lambda, self.num_label)
        return (torch.ones(b, 1, 1, 1), _collate_pcm(rows, self.sample_rate), torch.zeros(b, 1, dtype=torch.int64), labels,
                [it["name"] for it in items])


def build_audioset_clf_dataloader(cfg, data_name, label_map, shuffle=True, train=True, filters=None, decode_audio=None, echo=None):
    """audioset_clf.py:154-194 -> (sampler, loader).  `running.weighted_sampling` when training and without replicas: a
    WeightedRandomSampler over the dataset's `sample_weights`, with replacement, one epoch = len(dataset) draws."""
    rcfg = cfg.running
    weighted = bool(train and rcfg.get("weighted_sampling", False))
    dataset = AudiosetSrc(rcfg, data_name, train, label_map, weighted, filter_set=filters, decode_audio=decode_audio,
                          seed=int(cfg.seed), echo=echo)
    sampler = None
    if weighted:
        sampler = data.WeightedRandomSampler(dataset.sample_weights, len(dataset), replacement=True)
    return _loader(cfg, dataset, TaggingCollator(dataset.sample_rate, dataset.num_label), shuffle, sampler=sampler)
