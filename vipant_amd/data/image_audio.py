"""The image-audio dataset that reads raw files (cvap/data/image_audio.py:90-222 `ImageAudioDatasetSrc`, builder :333-375), in the
form the device front-ends want: a worker decodes containers only -- WAV to int16, JPEG / PNG to uint8 (decode.py) -- and the batch
carries the decoded bytes; waveform, log-mel, augmentation and image transform run on the GPU in the trainer's `make_batch`.
`running.multi_view` selects the siamese form (:224-305 `ImageAudioDatasetSiameseSrc`): the same payload once, six slots, and
markers where the reference stores second copies.

Host only: nothing here imports the HIP binding, calls torch.cuda or returns a device tensor -- a loader worker must never open the
GPU.  Index, path, frame-choice and fallback rules are the reference's; the deviations: a clip whose sample
rate differs from `running.sample_rate` is refused (one batched filter-bank launch has one rate), the random choices come from a
per-item generator seeded by (seed, index, epoch) instead of the worker's numpy state -- so a batch does not depend on the number
of workers --, and the `train_samples` subset is a seeded permutation.
"""
from __future__ import annotations

import json
import math
import os
import warnings

import numpy as np
import torch
import torch.utils.data as data

from ..errors import VipantError
from .decode import read_frame, read_wav


class FrameBatch:
    """Decoded frames of a batch: frames uint8 [b, Hmax, Wmax, 3] (frame i in the top left hw[i] pixels, zero elsewhere) and hw int32
    [b, 2].  `to` moves the frames; hw stays on the host, where the image views' launch reads it."""

    def __init__(self, frames, hw):
        self.frames, self.hw = frames, hw

    def to(self, device, non_blocking=False):
        return FrameBatch(self.frames.to(device, non_blocking=non_blocking), self.hw)

    def pin_memory(self):
        return FrameBatch(self.frames.pin_memory(), self.hw)

    @property
    def shape(self):
        return self.frames.shape


class PcmBatch:
    """Decoded clips of a batch: pcm int16 [b, stride] (clip i = nframes[i] frames of channels[i] interleaved samples, zero padded;
    stride = the batch maximum of frames x channels rounded up to 8), nframes int64 [b], channels int32 [b], and the sample rate."""

    def __init__(self, pcm, nframes, channels, sample_rate):
        self.pcm, self.nframes, self.channels, self.sample_rate = pcm, nframes, channels, int(sample_rate)

    def to(self, device, non_blocking=False):
        return PcmBatch(self.pcm.to(device, non_blocking=non_blocking), self.nframes.to(device, non_blocking=non_blocking),
                        self.channels.to(device, non_blocking=non_blocking), self.sample_rate)

    def pin_memory(self):
        return PcmBatch(self.pcm.pin_memory(), self.nframes.pin_memory(), self.channels.pin_memory(), self.sample_rate)

    @property
    def shape(self):
        return self.pcm.shape


class ImageAudioSrc(data.Dataset):
    """`__getitem__` decodes one (frame, clip) pair from disk -> {"frame": uint8 [h, w, 3] | "embed": fp32 [E], "pcm": int16 [n, ch],
    "name": id}.  `rcfg` = the `running` node.  decode_audio(path) -> (int16 [n, ch], rate) and decode_frame(path) -> uint8
    [h, w, 3] replace the WAV / PIL decoders (a FLAC reader, say)."""

    def __init__(self, rcfg, data_name, train, decode_audio=None, decode_frame=None, seed=0):
        data_path = f"{rcfg.data_root}/{data_name}.csv"
        if not os.path.isfile(data_path):
            raise VipantError(f"{data_path} is not a file.")
        self.dataset = []
        with open(data_path, "r") as fr:
            for iline, line in enumerate(fr):
                self.dataset.append(json.loads(line))
                if not train and iline + 1 == rcfg.eval_samples:
                    break
        if not self.dataset:
            raise VipantError(f"{data_path} holds no record.")
        self.seed, self.epoch = int(seed), 0
        fraction = float(rcfg.get("train_samples", 1.0))
        if train and 0.0 < fraction < 1.0:
            k = int(len(self.dataset) * fraction)
            order = torch.randperm(len(self.dataset), generator=torch.Generator().manual_seed(self.seed)).tolist()
            self.dataset = [self.dataset[i] for i in order[:k]]
        # compatible with AudioSet and Balanced AudioSet (image_audio.py:110)
        self.aclip_key = "clip" if "clip" in self.dataset[0] else "aclip"
        self.frame_key = rcfg.frame_key
        self.length, self.train = len(self.dataset), bool(train)
        self.data_root, self.frame_emb = str(rcfg.data_root), rcfg.get("frame_emb", None)
        res = rcfg.get("resolution", 224)
        self.resolution = 224 if isinstance(res, (list, tuple)) or res is None else int(res)
        self.embed_dim = int(rcfg.get("embed_dim", 512))
        self.sample_rate = int(rcfg.get("sample_rate", 16000))
        self.decode_audio = decode_audio if decode_audio is not None else read_wav
        self.decode_frame = decode_frame if decode_frame is not None else read_frame

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def _generator(self, index):
        """The item's own generator: the training draws of item `index` in epoch `epoch` (evaluation draws nothing that varies)."""
        return torch.Generator().manual_seed(self.seed + 13 + int(index) + 1000003 * (self.epoch if self.train else 0))

    def _process_item(self, index, generator=None, frames=True):
        """image_audio.py:131-151 -> (name, clip file, frame file, frame embedding file or None).  `frames=False` (a dataset that
        shows no image: audio_text.py): the clip alone, the record's frames are not read and nothing is drawn."""
        record = self.dataset[index]
        name, sub = record["id"], record.get("dir", "")
        base = f"{self.data_root}/{sub}/" if sub else f"{self.data_root}/"            # a record without `dir` reads from the root
        clip_file = f"{base}{self.aclip_key}/{name}.{record[self.aclip_key][0]}"        # the first extension listed
        if not frames:
            return name, clip_file, None, None
        frame, embed_file = record[self.frame_key], None
        if not isinstance(frame, str):                                                 # a list of frame names: pick one
            if self.train:
                generator = generator if generator is not None else self._generator(index)
                pick = int(torch.randint(len(frame), (1,), generator=generator))
            else:
                pick = int(math.ceil(len(frame) / 2)) - 1                              # the middle frame, the lower one of two
            frame = frame[pick]
            if self.frame_emb is not None:                                             # (only a listed frame has an embedding file)
                embed_file = f"{self.data_root}/{self.frame_emb}/{name}.{frame.rsplit('.', 1)[0]}.npz"
        return name, clip_file, f"{base}{self.frame_key}/{name}.{frame}", embed_file

    def _embed(self, fname, generator):
        try:
            return np.asarray(np.load(fname)["v"], dtype=np.float32)
        except Exception as e:
            warnings.warn(f"use random image instead because `{e}` {fname}.")
            return torch.rand(self.embed_dim, generator=generator).numpy()

    def _frame(self, fname, generator):
        try:
            frame = np.asarray(self.decode_frame(fname))
            if frame.dtype != np.uint8 or frame.ndim != 3 or frame.shape[2] != 3:
                raise VipantError(f"the decoder returned {frame.dtype} {frame.shape}, not uint8 [h, w, 3]")
            return frame
        except Exception as e:
            h = w = self.resolution
            warnings.warn(f"use random image instead because `{e}` {fname}.")
            return torch.randint(0, 256, (h, w, 3), generator=generator, dtype=torch.uint8).numpy()

    def _pcm(self, fname):
        pcm, rate = self.decode_audio(fname)
        pcm = np.asarray(pcm)
        if pcm.ndim == 1:
            pcm = pcm[:, None]
        if pcm.dtype != np.int16 or pcm.ndim != 2:
            raise VipantError(f"{fname}: the decoder returned {pcm.dtype} {pcm.shape}, not int16 [n, ch]")
        if int(rate) != self.sample_rate:
            raise VipantError(f"{fname}: sample rate {int(rate)} Hz, but running.sample_rate = {self.sample_rate} "
                              "(there is no resampling: one batched filter-bank launch has one rate)")
        return np.ascontiguousarray(pcm)

    def __getitem__(self, index):
        g = self._generator(index)
        name, aclip_file, frame_file, frame_emb_file = self._process_item(index, g)
        item = {"name": name}
        if frame_emb_file is not None:          # higher priority for pre-computed frame embeddings (image_audio.py:212-213)
            item["embed"] = self._embed(frame_emb_file, g)
        else:
            item["frame"] = self._frame(frame_file, g)
        item["pcm"] = self._pcm(aclip_file)     # a clip that cannot be decoded raises
        return item

    def __len__(self):
        return self.length


class ImageAudioSiameseSrc(ImageAudioSrc):
    """The siamese trainer's dataset (cvap/data/image_audio.py:224-305 `ImageAudioDatasetSiameseSrc`): two views of one frame and two
    views of one clip.  Both views of a modality are made on the device from ONE decoded payload, so an item holds the decoded
    frame and the PCM once -- {"frame": uint8 [h, w, 3], "pcm": int16 [n, ch], "name": id} -- and, when a loss pair reads the
    pre-computed frame embedding (`model.loss.vp or model.loss.ap`, :290), {"embed": fp32 [E]} as well.  A record whose frame is a
    single name has no embedding file: its embedding is the random vector under the reference's warning.  `cfg` = the whole
    configuration (`running` and `model.loss`)."""

    def __init__(self, cfg, data_name, train, decode_audio=None, decode_frame=None, seed=0):
        super().__init__(cfg.running, data_name, train, decode_audio=decode_audio, decode_frame=decode_frame, seed=seed)
        if self.frame_emb is None:              # image_audio.py:231
            raise VipantError("running.frame_emb is None: the siamese src dataset expects the directory of the frame embeddings")
        lcfg = cfg.model.loss
        self.with_embed = bool(lcfg.get("vp", False) or lcfg.get("ap", False))

    def __getitem__(self, index):
        g = self._generator(index)
        name, aclip_file, frame_file, frame_emb_file = self._process_item(index, g)
        item = {"name": name}
        if self.with_embed:
            item["embed"] = self._embed(frame_emb_file, g)
        item["frame"] = self._frame(frame_file, g)
        item["pcm"] = self._pcm(aclip_file)
        return item


class SecondView:
    """The second view slot of a siamese batch: it holds no data of its own, only the index of the slot whose payload it is a view of
    (the frames and the PCM of a batch cross the worker boundary, and later the bus to the device, once)."""

    def __init__(self, of):
        self.of = int(of)

    def to(self, device, non_blocking=False):
        return self

    def pin_memory(self):
        return self


def _collate_frames(items):
    b = len(items)
    hw = torch.tensor([[it["frame"].shape[0], it["frame"].shape[1]] for it in items], dtype=torch.int32)
    frames = torch.zeros((b, int(hw[:, 0].max()), int(hw[:, 1].max()), 3), dtype=torch.uint8)
    for i, it in enumerate(items):
        frames[i, :int(hw[i, 0]), :int(hw[i, 1])] = torch.from_numpy(np.ascontiguousarray(it["frame"]))
    return FrameBatch(frames, hw)


def _collate_pcm(items, sample_rate):
    b = len(items)
    nframes = torch.tensor([it["pcm"].shape[0] for it in items], dtype=torch.int64)
    channels = torch.tensor([it["pcm"].shape[1] for it in items], dtype=torch.int32)
    stride = max(8, -(-int((nframes * channels).max()) // 8) * 8)
    pcm = torch.zeros((b, stride), dtype=torch.int16)
    for i, it in enumerate(items):
        flat = torch.from_numpy(np.ascontiguousarray(it["pcm"]).reshape(-1))
        pcm[i, :flat.numel()] = flat
    return PcmBatch(pcm, nframes, channels, sample_rate)


class SrcCollator:
    """Items -> the trainers' five-slot tuple (images, audios, text, labels, names): images a FrameBatch (or fp32 [b, E] embeddings),
    audios a PcmBatch, text int64 [b, 1] zeros and labels int64 [b] zeros as the synthetic loader yields them without text.
    Everything is on the CPU."""

    def __init__(self, sample_rate=16000):
        self.sample_rate = int(sample_rate)

    def __call__(self, items):
        b = len(items)
        if all("embed" in it for it in items):
            images = torch.from_numpy(np.stack([np.asarray(it["embed"], dtype=np.float32) for it in items]))
        elif all("frame" in it for it in items):
            images = _collate_frames(items)
        else:
            raise VipantError("a batch mixes frames and frame embeddings (records with a single frame name have no embedding file)")
        audios = _collate_pcm(items, self.sample_rate)
        return (images, audios, torch.zeros(b, 1, dtype=torch.int64), torch.zeros(b, dtype=torch.int64),
                [it["name"] for it in items])


class SiameseSrcCollator:
    """Items of ImageAudioSiameseSrc -> the siamese trainer's six slots (image, image_v1, image_v2, audio_v1, audio_v2, names), as
    the reference's collator orders them (image_audio.py:317-325): image fp32 [b, E] embeddings, or the reference's [b, 1, 1, 1] ones
    when no loss pair reads them; image_v1 a FrameBatch and audio_v1 a PcmBatch; image_v2 and audio_v2 SecondView markers of slots
    1 and 3.  Everything is on the CPU."""

    def __init__(self, sample_rate=16000):
        self.sample_rate = int(sample_rate)

    def __call__(self, items):
        if all("embed" in it for it in items):
            image = torch.from_numpy(np.stack([np.asarray(it["embed"], dtype=np.float32) for it in items]))
        else:
            image = torch.ones(len(items), 1, 1, 1)
        return (image, _collate_frames(items), SecondView(1), _collate_pcm(items, self.sample_rate), SecondView(3),
                [it["name"] for it in items])


def build_image_audio_dataloader(cfg, data_name, shuffle=True, train=True, decode_audio=None, decode_frame=None):
    """image_audio.py:333-375 -> (sampler, loader).  Under replicas every rank takes its share through a DistributedSampler and
    `running.batch_size` is the per-rank batch (one process per GPU)."""
    rcfg = cfg.running
    data_name = str(data_name)
    if data_name.startswith("npz"):
        raise VipantError("npz datasets: not built")
    if not data_name.startswith("src") or str(rcfg.data_root).startswith("gs://"):
        raise VipantError(f"unrecognized dataset `{data_name}`.")
    if rcfg.get("multi_view", False):
        dataset = ImageAudioSiameseSrc(cfg, data_name, train, decode_audio=decode_audio, decode_frame=decode_frame, seed=int(cfg.seed))
        collator = SiameseSrcCollator(dataset.sample_rate)
    else:
        dataset = ImageAudioSrc(rcfg, data_name, train, decode_audio=decode_audio, decode_frame=decode_frame, seed=int(cfg.seed))
        collator = SrcCollator(dataset.sample_rate)
    replicas = torch.distributed.is_available() and torch.distributed.is_initialized()
    if replicas:
        sampler = data.distributed.DistributedSampler(dataset, shuffle=shuffle, drop_last=True)
    else:
        sampler = data.RandomSampler(dataset) if shuffle else data.SequentialSampler(dataset)
    workers = int(cfg.get("num_proc", 0) or 0)
    loader = data.DataLoader(
        dataset, batch_size=int(rcfg.batch_size), collate_fn=collator, num_workers=workers, pin_memory=True,
        sampler=sampler, drop_last=bool(replicas),
        # spawn: a forked worker would inherit the parent's open device
        multiprocessing_context=("spawn" if workers > 0 else None))
    return sampler, loader
