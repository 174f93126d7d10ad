"""Trainer loop with the reference's Monitor contract (`Monitor(cfg, echo, device).learn()`), reproducing
the step semantics of VALMonitor.epoch / VAMonitor.epoch (cvap/monitor/cvalp.py:172-272, cvap/monitor/cvap.py:160-244):
per step -- H2D, LARS learning-rate schedule, zero_grad(set_to_none), forward, backward, optimizer step, counters,
`samples/s` log line, periodic eval + checkpoint.

Deliberate deviations (documented in DESIGN.md):
  * bf16 MFMA operands with fp32 accumulation and an fp32 residual stream need no loss scaling, so the reference's
    fp16 autocast + GradScaler pair (cvalp.py:123, 201-205) has no counterpart here;
  * one process per GPU: `mode=ddp` is served by vipant_amd.parallel (feature all-gather + bucketed gradient
    all-reduce); the reference's ddp branch cannot start (train.py:35 names an undefined Monitor);
  * with `running.data_root` empty (the default) batches come from a synthetic loader with the reference's tensor contract,
    unless a loader is injected through `dataloader=`.  With `running.data_root=DIR` the bimodal VA trainer reads the reference's
    raw-file image-audio dataset (vipant_amd/data, cvap/data/image_audio.py:90-222): loader workers decode containers only, and
    `make_batch` runs waveform, log-mel, augmentation and image transform on the device; under
    `running.multi_view` the siamese trainer reads the siamese form of that dataset (cvap/data/image_audio.py:224-305; section 18);
    the AT trainer reads the caption datasets (`data_name=audiocaps*` / `clotho*`: cvap/data/audiocaps.py, audio_text.py; section
    19), without the AudioSet label map; the x-fold trainer reads ESC-50 / UrbanSound8K and the tagging trainer the AudioSet clf
    dataset with its label map, filter set and dataset-wide mixup partners (cvap/data/esc50.py, audioset_cls.py, audioset_hub.py;
    section 20); the reference's other dataset builders are not built.
"""
from __future__ import annotations

import os
import time
from collections import defaultdict

import numpy as np
import torch

from . import parallel
from ._ffi import VipantError
from .data import FrameBatch, PcmBatch, SecondView
from .model import build_main_model
from .module import LARS, adjust_learning_rate, exclude_bias_or_norm

SOT, EOT = 49406, 49407


class SyntheticLoader:
    """Batches with the tensor contract of the reference collators (cvap/data/audioset_clf.py:122-152,
    cvap/monitor/cvalp.py:136-154): (images, audios [b, T, F], text [b, L] i64, labels, names).  Seeded per rank and
    per step, reproducible.  `running.dp_chunk` (set by train.py for `mode=dp` under N replicas): the loader
    stands for the reference's ONE loader whose batch data_parallel scatters -- every replica draws the same global batch of
    N x batch_size samples and keeps its contiguous chunk.
    `running.multi_view` (configs/running/siamese.yaml): the five-slot batch of the siamese VA trainer instead -- (prime image
    features [b, E], image view 1, image view 2 [b, 3, res, res], audio view 1, audio view 2 [b, T, F], names); the two views of a
    modality are one clip under independent noise.
    `running.image_frames: [H, W]` (opt-in): the image slot holds decoded FRAMES uint8 [b, H, W, 3] instead, as a loader that
    leaves the image transform to the device yields them (vipant_amd/image_views.py); under `multi_view` the same frames fill both
    view slots -- one frame gives two views, as in the reference (cvap/data/image_audio.py:232-237)."""

    def __init__(self, cfg, steps, with_text, device_rank=0):
        self.cfg, self.steps, self.with_text, self.rank = cfg, int(steps), with_text, device_rank
        rcfg = cfg.running
        self.b = int(rcfg.batch_size)
        self.chunk = None
        if rcfg.get("dp_chunk", False) and parallel.world_size() > 1:
            self.chunk = (parallel.rank(), self.b)
            self.b, self.rank = self.b * parallel.world_size(), 0
        self.T, self.F = int(rcfg.max_audio_len), int(rcfg.num_mel_bins)
        self.precomputed = bool(rcfg.get("precomputed_image", False)) or rcfg.get("frame_emb", None) is not None
        self.res = int(cfg.running.resolution) if not isinstance(cfg.running.resolution, (list, tuple)) else 224
        self.embed = int(cfg.running.embed_dim)
        self.multi_view = bool(rcfg.get("multi_view", False))
        frames = rcfg.get("image_frames", None)
        self.image_frames = (int(frames[0]), int(frames[1])) if frames else None

    def _frames(self, step):
        g = torch.Generator().manual_seed(77003 + 1000 * self.rank + step)      # a generator of their own: the other slots keep their draws
        return torch.randint(0, 256, (self.b, *self.image_frames, 3), generator=g, dtype=torch.uint8)

    def __len__(self):
        return self.steps

    def __iter__(self):
        for step in range(self.steps):
            g = torch.Generator().manual_seed(1213 + 1000 * self.rank + step)
            audios = torch.randn(self.b, self.T, self.F, generator=g)
            if self.multi_view:
                frames = torch.randn(self.b, 3, self.res, self.res, generator=g)
                batch = (torch.randn(self.b, self.embed, generator=g),
                         frames + 0.5 * torch.randn(frames.shape, generator=g), frames + 0.5 * torch.randn(frames.shape, generator=g),
                         audios + 0.5 * torch.randn(audios.shape, generator=g), audios + 0.5 * torch.randn(audios.shape, generator=g))
                if self.image_frames:
                    u8 = self._frames(step)
                    batch = (batch[0], u8, u8, batch[3], batch[4])
                names = [f"synthetic-{self.rank}-{step}-{i}" for i in range(self.b)]
                if self.chunk is not None:
                    sl = slice(self.chunk[0] * self.chunk[1], (self.chunk[0] + 1) * self.chunk[1])
                    batch, names = tuple(t[sl] for t in batch), names[sl]
                yield (*batch, names)
                continue
            if self.with_text:
                images = torch.zeros(self.b, 1, 1, 1)
                lens = torch.randint(8, 78, (self.b,), generator=g)
                L = int(lens.max())
                text = torch.zeros(self.b, L, dtype=torch.int64)
                for i in range(self.b):
                    n = int(lens[i])
                    text[i, 0] = SOT
                    text[i, 1:n - 1] = torch.randint(1, SOT, (n - 2,), generator=g)
                    text[i, n - 1] = EOT
            else:
                images = (torch.randn(self.b, self.embed, generator=g) if self.precomputed
                          else torch.randn(self.b, 3, self.res, self.res, generator=g))
                text = torch.zeros(self.b, 1, dtype=torch.int64)
                if self.image_frames and not self.precomputed:
                    images = self._frames(step)
            labels = torch.zeros(self.b, dtype=torch.int64)
            names = [f"synthetic-{self.rank}-{step}-{i}" for i in range(self.b)]
            if self.chunk is not None:
                sl = slice(self.chunk[0] * self.chunk[1], (self.chunk[0] + 1) * self.chunk[1])
                images, audios, text, labels, names = images[sl], audios[sl], text[sl], labels[sl], names[sl]
            yield images, audios, text, labels, names


def _synthetic_prompts(seed, nclass):
    """One tokenised prompt per class (`running.prompt` + label): SOT, ids, EOT, zero-padded to a common width."""
    g = torch.Generator().manual_seed(seed)
    prompts = []
    for c in range(nclass):
        n = int(torch.randint(3, 8, (1,), generator=g))
        prompts.append([SOT] + torch.randint(1, SOT, (n,), generator=g).tolist() + [EOT])
    width = max(len(t) for t in prompts)
    return [t + [0] * (width - len(t)) for t in prompts]


class Monitor(object):
    with_text = True      # VALMonitor (AT); VAMonitor sets False
    partial_head_grads = False      # a classification head scores a rank's own rows: its gradients join the replica reduction
    norms_only = False              # `running.audio.eval_norms` on a file dataset: the statistics are the run's only task

    def __init__(self, cfg, echo, device, dataloader=None):
        self.cfg, self.echo, self.device = cfg, echo, device
        self.evalloader = self.testloader = None
        self.gold_file = None
        self.model = None
        self.dataloader = dataloader if dataloader is not None else self.build_data()
        acfg = cfg.running.get("audio", None) or {}
        self.norms_only = dataloader is None and self._from_files() and bool(acfg.get("eval_norms", False))
        if self.norms_only:
            self.eval_norms()
            return      # mean & std of the data: the only task of such a run (cvap.py:28-30)
        model = build_main_model(cfg, echo)
        negatives = cfg.running.get("negatives", "global")
        tunable_params = model.build(negatives=negatives)
        self.model = model
        self._configure(model)
        self.model.train(not cfg.eval)
        self.build_optimizer(tunable_params)

    def _configure(self, model):
        """Run-time switches of the towers (`running.*`) and, under replicas, the gradient reduction they feed."""
        cfg = self.cfg
        towers = (model.audio_head, getattr(model, "image_head", None), getattr(model, "text_head", None))
        self.grad_sync = None
        if parallel.active():
            # `running.comm_overlap`: block (default: each block's bucket is reduced while the blocks below run their backward) | step
            self.grad_sync = parallel.GradSync(overlap=str(cfg.running.get("comm_overlap", "block")))
            for head in towers:
                if head is not None and hasattr(head, "encoder"):
                    head.encoder.grad_sync = self.grad_sync
        if cfg.running.get("recompute_mlp", False):
            for head in towers:
                if head is not None and hasattr(head, "encoder"):
                    head.encoder.recompute_mlp = True
        if cfg.running.get("grad_stream", None) is not None:        # bf16 (default) | fp32 master of the stream gradient
            from . import ops
            ops.GRAD_STREAM_F32 = str(cfg.running.grad_stream).lower() in ("fp32", "float32")
        # the residual stream inside every transformer stack: fp16 (the reference's autocast precision; default) or fp32;
        # LayerNorm statistics are fp32 either way
        stream_f16 = str(cfg.running.get("stream_dtype", "fp16")).lower() in ("fp16", "float16", "half")
        # `running.last_block_rows` (default on): a tower's last block is evaluated on the rows its read-out takes (class / end-of-text
        # token) -- exact, see ops.BackboneFn; off: the full block, as the reference computes it before discarding the other rows
        last_rows = bool(cfg.running.get("last_block_rows", True)) and os.environ.get("VIPANT_LAST_BLOCK_ROWS", "1") != "0"
        for head in towers:
            if head is not None and hasattr(head, "encoder"):
                head.encoder.stream_f16 = stream_f16
                head.encoder.last_block_rows = last_rows
        # (audio tower only: a trainable image tower -- worker=CVASP, model.image.freeze=False -- runs bf16 operands)
        if cfg.running.get("fp8_gemm", False):      # BASELINE.json configs[4]: e4m3 operands in the audio tower's NT contractions
            if model.audio_head is not None and hasattr(model.audio_head, "encoder"):
                model.audio_head.encoder.fp8 = True

    def _from_files(self):
        return bool(self.cfg.running.get("data_root", "") or "")

    def build_data(self):
        rcfg = self.cfg.running
        if self._from_files():
            return self.build_file_data()
        steps = rcfg.get("synthetic_steps", 8)
        loader = SyntheticLoader(self.cfg, steps, self.with_text, max(self.cfg.rank, 0))
        self.echo(f"Instantiate main dataloader from `synthetic': total {len(loader)} batches.")
        return loader

    # ------------------------------------------------------------------ cvap.py:67-87
    def build_file_data(self):
        """`running.data_root=DIR`: the raw-file image-audio dataset, and when training the evaluation loader if its index exists
        (a trainer with text: the caption datasets, `build_caption_data`)."""
        from .data import build_image_audio_dataloader
        rcfg = self.cfg.running
        if self.with_text:
            return self.build_caption_data()
        data_name = rcfg.eval_name if self.cfg.eval else rcfg.data_name
        _, loader = build_image_audio_dataloader(self.cfg, data_name, shuffle=(not self.cfg.eval), train=(not self.cfg.eval))
        nstep = len(loader)
        if nstep < rcfg.peep_rate:
            rcfg.peep_rate = nstep
        self.echo(f"Instantiate main dataloader from `{data_name}': total {nstep} ({rcfg.peep_rate}) batches.")
        self.gold_file = f"{rcfg.data_root}/{data_name}.csv"
        eval_name = "" if self.cfg.eval else rcfg.eval_name
        if eval_name and os.path.isfile(f"{rcfg.data_root}/{eval_name}.csv"):
            _, self.evalloader = build_image_audio_dataloader(self.cfg, eval_name, shuffle=False, train=False)
            self.echo(f"Will do evaluation every {rcfg.save_rate} steps on {len(self.evalloader)} batches.")
            self.gold_file = f"{rcfg.data_root}/{eval_name}.csv"
        return loader

    # ------------------------------------------------------------------ cvalp.py:65-104
    def build_caption_data(self):
        """`running.data_root=DIR` under a trainer with text: the caption datasets (vipant_amd/data/audio_text.py; `audiocaps*`,
        `clotho*`), and when training the evaluation and the test loader whose index exists.  No label map: the reference builds one
        from AudioSet ontology files that the caption datasets never read."""
        from .data import build_audio_text_dataloader
        rcfg = self.cfg.running
        data_name = str(rcfg.eval_name if self.cfg.eval else rcfg.data_name)
        if data_name.startswith(("src", "npz")):
            raise VipantError(f"running.data_name=`{data_name}` under monitor=VALMonitor: the AudioSet datasets with text are not built; "
                              "the data names that work here begin with `audiocaps` or `clotho`")
        _, loader = build_audio_text_dataloader(self.cfg, data_name, shuffle=(not self.cfg.eval), train=(not self.cfg.eval))
        nstep = len(loader)
        if nstep < rcfg.peep_rate:
            rcfg.peep_rate = nstep
        self.echo(f"Instantiate main dataloader from `{data_name}': total {nstep} batches.")
        self.gold_file = f"{rcfg.data_root}/{data_name}.csv"

        def side_loader(name):
            name = "" if self.cfg.eval else str(name or "")
            if not name or not os.path.isfile(f"{rcfg.data_root}/{name}.csv"):
                return None
            return build_audio_text_dataloader(self.cfg, name, shuffle=False, train=False)[1]
        self.evalloader = side_loader(rcfg.eval_name)
        if self.evalloader is not None:
            self.echo(f"Will do evaluation every {rcfg.save_rate} steps on {len(self.evalloader)} batches ({rcfg.eval_name}).")
            self.gold_file = f"{rcfg.data_root}/{rcfg.eval_name}.csv"
        self.testloader = side_loader(rcfg.test_name)
        if self.testloader is not None:
            self.echo(f"Will do test every {rcfg.save_rate} steps on {len(self.testloader)} batches ({rcfg.test_name}).")
            self.gold_file_test = f"{rcfg.data_root}/{rcfg.test_name}.csv"
        return loader

    # ------------------------------------------------------------------ cvap.py:43-65
    def eval_norms(self):
        """`running.audio.eval_norms=True`: mean and standard deviation of the main loader's log-mels, norms and every augmentation
        off (KaldiFbank.from_config switches them off under the key) -- the `running.audio.norms` of a new dataset.  Per clip the
        mean and the mean square over [T, F], in float64; then their means over the clips."""
        self.echo("Evaluate mean and std...")
        som_list, sos_list = [], []
        for step, batch in enumerate(self.dataloader):
            audios = self.make_batch(batch)[1].double()
            som_list.append(audios.mean(dim=[2, 3]))
            sos_list.append((audios ** 2).mean(dim=[2, 3]))
            self.echo(f"step {step}")
        som = torch.cat(som_list, 0).mean(dim=[0])
        sos = torch.cat(sos_list, 0).mean(dim=[0])
        std = (sos - som ** 2).sqrt()
        self.norms = (som.cpu().tolist(), std.cpu().tolist())
        self.echo(f"MEAN: {self.norms[0]} STD: {self.norms[1]}")

    def _training(self):
        return bool(self.model.training) if self.model is not None else not self.cfg.eval

    # ------------------------------------------------------------------ cvalp.py:106-130
    def learn(self):
        if self.norms_only:
            return None
        if not self.model.training:
            self.echo("Evaluating started...")
            with torch.no_grad():
                report = self.infer(self.dataloader, samples=self.cfg.running.eval_samples, gold_file=self.gold_file)
                self.echo(f"{report}")
                return None
        self.echo("Training started...")
        self.last_time = 0.
        self.total_loss = 0
        self.total_step = 0
        self.total_inst = 0
        self.start_time = time.time()
        for iepoch in range(int(self.cfg.optimizer.epochs)):
            self.epoch(iepoch)

    # ------------------------------------------------------------------ cvalp.py:136-154
    def image_views(self, images, which="prime", siamese=False, hw=None):
        """A uint8 image slot [b, H, W, 3] (decoded frames) -> the tower's input, on the device (vipant_amd/image_views.py): `clip`
        unless this is a training view of the siamese trainer without `running.clip_tf`; then `barlow`, with its draws from the
        per-rank host generator, consumed in step order.  Anything else passes through.  hw [b, 2] on the host: the (h, w) of each
        frame inside the canvas (default: all of it)."""
        if images is None or images.dtype != torch.uint8 or images.dim() != 4:
            return images
        from .image_views import ImageViews
        cache = self.__dict__.setdefault("_image_views", {})
        key = (self._training(), which, siamese)
        if key not in cache:
            cache[key] = ImageViews.from_config(self.cfg.running, train=key[0], which=which, device=self.device, siamese=siamese)
        iv = cache[key]
        if iv.chain == "clip":
            return iv(images, hw=hw)
        if "_image_generator" not in self.__dict__:
            self._image_generator = self._image_views_generator()
        if hw is None:
            hw = [[images.shape[1], images.shape[2]]] * images.shape[0]
        return iv(images, hw=hw, draws=iv.draw_image_views(hw, self._image_generator))

    def _image_views_generator(self):
        return torch.Generator().manual_seed(int(self.cfg.seed) + 11 + 1000 * max(int(self.cfg.rank), 0))

    def _aug_generator(self):
        """The host generator of the waveform-view and SpecAugment draws: seeded per rank, consumed in step order."""
        return torch.Generator().manual_seed(int(self.cfg.seed) + 7 + 1000 * max(int(self.cfg.rank), 0))

    def pcm_frontend(self, train, sample_rate):
        from .frontend import KaldiFbank
        cache = self.__dict__.setdefault("_pcm_fbank", {})
        key = (bool(train), int(sample_rate))
        if key not in cache:
            cache[key] = KaldiFbank.from_config(self.cfg.running.audio, float(sample_rate), train=train, device=self.device)
        return cache[key]

    def audios_from_pcm(self, clips, tile=None):
        """A PcmBatch (decoded 16-bit clips, on the host) -> log-mels [b, 1, T, F] on the device, in the reference's order
        (image_audio.py:183-207, transform.py:15-35): H2D, the waveform (`pcm_wave`: channel rule, `tile_audio`), then inside the
        log-mel launch the `audio_transforms` chain and the crop rule, the filter bank, `norms`, and the SpecAugment masks.  Training
        draws views when there is a chain or a clip longer than `crop_len`, and masks under `transform_fbank`; evaluation takes the
        centred crop of a longer clip and nothing else; `eval_norms` switches chain, masks and norms off.  `tile`: None follows
        `running.audio.tile_audio`; False never tiles (the x-fold datasets pass `tile_audio=False` whatever the key says, esc50.py:81)."""
        from .frontend import pcm_wave
        acfg = self.cfg.running.audio
        train = self._training()
        fbank = self.pcm_frontend(train, clips.sample_rate)
        tile = bool(acfg.get("tile_audio", False)) if tile is None else bool(tile)
        tile_len = int(fbank.max_len / 100 * clips.sample_rate) if tile else 0
        # the lengths pcm_wave will report, from the host's copy (no device sync)
        n = torch.minimum(clips.nframes, clips.pcm.shape[1] // clips.channels.clamp(1, 8).long()).clamp_(min=0)
        if tile_len > 0:
            n = torch.where((n > 0) & (n < tile_len), n * ((tile_len + n - 1) // n.clamp(min=1)), n)
        longest = int(n.max())
        on_dev = clips.to(self.device, non_blocking=True)
        wave, nsamples = pcm_wave(on_dev.pcm, on_dev.nframes, on_dev.channels, mode=str(acfg.get("channel", "first")),
                                  tile_len=tile_len, wave_stride=max(8, -(-longest // 8) * 8))
        if "aug_generator" not in self.__dict__:
            self.aug_generator = self._aug_generator()
        b, view = wave.shape[0], None
        crop = longest > fbank.crop_len
        if train and (fbank.chain or crop):
            view = fbank.draw_views(b, self.aug_generator)
        elif crop:
            view = True                                                    # evaluation: the centred window and its rule
        masks = fbank.draw_masks(b, self.aug_generator) if train else None
        return fbank(wave, nsamples, masks=masks, view=view)

    def make_batch(self, batch):
        if isinstance(batch[0], FrameBatch):
            images = self.image_views(batch[0].frames.to(self.device, non_blocking=True), hw=batch[0].hw)
        else:
            images = self.image_views(torch.as_tensor(batch[0]).to(self.device, non_blocking=True))
        if isinstance(batch[1], PcmBatch):
            audios = self.audios_from_pcm(batch[1])
        else:
            audios = torch.as_tensor(batch[1]).to(self.device, non_blocking=True).unsqueeze(1)
        text = torch.as_tensor(batch[2]).to(self.device, non_blocking=True)
        labels = torch.as_tensor(batch[3]).to(self.device, non_blocking=True)
        return images, audios, text, labels, batch[-1]

    def timeit(self, time_dict, key=None, show=False):
        if self.cfg.rank > 0:
            return
        if show:
            report = " ".join(f"{k} {np.mean(v):.2f}" for k, v in time_dict.items())
            self.echo(f"Time (s): {report}; # step {self.total_step} # sample {self.total_inst}")
            return
        if key is None:
            self.last_time = time.time()
        else:
            this_time = time.time()
            time_dict[key].append(this_time - self.last_time)
            self.last_time = this_time

    # ------------------------------------------------------------------ one optimisation step
    def _forward_backward_micro(self, images, audios, text, mb):
        """One global-batch step with the towers run `mb` samples at a time (`running.micro_batch`), for batches whose
        activations do not fit at once (BASELINE.json configs[4]: ViT-L, 1024 clips per GPU).  The objective is untouched --
        every sample is still scored against the whole batch:
          1. features of all micro-batches, nothing kept for a backward;
          2. the loss over the concatenated features -> d loss / d features (and the loss head's own gradients);
          3. every micro-batch again, this time kept, and back-propagated from its slice of (2).
        The parameter gradients equal the one-pass gradients up to fp32 summation order; the price is one extra tower forward."""
        n = audios.shape[0]
        cuts = [(i, min(i + mb, n)) for i in range(0, n, mb)]
        parts = []
        with torch.no_grad():
            for a, b in cuts:
                parts.append(self.model.features(images[a:b], audios[a:b], text[a:b] if text is not None else None))
        feats = [None if parts[0][m] is None else torch.cat([p[m] for p in parts]).detach() for m in range(3)]
        heads = (self.model.image_head, self.model.audio_head, self.model.text_head)
        live = [m for m in range(3) if feats[m] is not None and heads[m] is not None
                and any(p.requires_grad for p in heads[m].parameters())]
        for m in live:
            feats[m].requires_grad_()
        loss = self.model.loss_from_features(*feats)
        loss.backward()
        if not live:                       # every tower frozen: only the loss head trains, nothing to re-run
            return loss
        # Pass 3 under data-parallel replicas: the per-block reduction buckets of the stacks are switched off for the micro-batches
        # -- each one would start a full set of all-reduces (n_micro x the traffic and n_micro flat gradient copies) -- autograd
        # accumulates locally instead and `step()` reduces the accumulated gradients ONCE (all parameters through reduce_params).
        # Towers that are frozen keep their pass-1 features: only the live modalities are run again.
        stacks = [h.encoder for h in heads if h is not None and hasattr(h, "encoder")]
        saved_sync = [st.grad_sync for st in stacks]
        for st in stacks:
            st.grad_sync = None
        try:
            for a, b in cuts:
                again = self.model.features(images[a:b] if 0 in live else None, audios[a:b] if 1 in live else None,
                                            text[a:b] if (2 in live and text is not None) else None)
                torch.autograd.backward([again[m] for m in live], [feats[m].grad[a:b] for m in live])
        finally:
            for st, gs in zip(stacks, saved_sync):
                st.grad_sync = gs
        self._micro_step = True
        return loss

    def step(self, images, audios, text):
        """zero_grad -> forward -> backward -> (replica gradient reduction) -> optimizer (cvalp.py:200-205)."""
        self.optimizer.zero_grad(set_to_none=True)
        mb = int(self.cfg.running.get("micro_batch", 0) or 0)
        if 0 < mb < audios.shape[0]:
            loss = self._forward_backward_micro(images, audios, text if self.with_text else None, mb)
        else:
            loss = self.model(images, audios, text if self.with_text else None)
            self._backward(loss)
        self._reduce_and_update()
        return loss

    @staticmethod
    def _backward(loss):
        from . import ops
        loss.backward(gradient=ops.unit_grad(loss.device) if loss.is_cuda and loss.dim() == 0 and loss.dtype == torch.float32 else None)

    def _reduce_and_update(self):
        """(replica gradient reduction) -> optimizer: the tail of every step."""
        if self.grad_sync is not None:
            micro = getattr(self, "_micro_step", False)         # micro-batched step: nothing went through a per-block bucket
            self._micro_step = False
            rest = [p for p in self.params if micro or not getattr(p, "_vipant_bucketed", False)]
            if (not self.partial_head_grads and self.model.loss_head is not None
                    and self.cfg.running.get("negatives", "global") == "global"):
                skip = {id(p) for p in self.model.loss_head.parameters()}      # complete on every rank already
                rest = [p for p in rest if id(p) not in skip]
            self.grad_sync.reduce_params(rest)      # one more bucket behind the per-block ones already in flight
            self.grad_sync.wait()
        self.optimizer.step()

    def _step_inputs(self, batch):
        """What `make_batch` returned -> (the arguments of `step`, the number of samples in the batch)."""
        images, audios, text, _, _ = batch
        return (images, audios, text), images.shape[0]

    # ------------------------------------------------------------------ cvalp.py:172-272
    def epoch(self, iepoch):
        all_time = defaultdict(list)
        self.timeit(all_time)
        nchunk = parallel.world_size()
        ocfg = self.cfg.optimizer
        warmup_step_rate = max(int(ocfg.warmup_steps) // 20, 1)      # cvalp.py:177
        for part in (getattr(self.dataloader, "dataset", None), getattr(self.dataloader, "sampler", None)):
            if hasattr(part, "set_epoch"):          # a file dataset's per-item draws and a DistributedSampler's order (cvap.py:107-108)
                part.set_epoch(iepoch)
        for step, batch in enumerate(self.dataloader, start=iepoch * len(self.dataloader)):
            inputs, ninst = self._step_inputs(self.make_batch(batch))
            self.timeit(all_time, key="data")
            if ocfg.use_lars:
                adjust_learning_rate(ocfg, self.optimizer, self.dataloader, step)
            # linear warm-up of a torch.optim optimizer (cvalp.py:185-198); always applied at the very first step
            warmup = (not ocfg.use_lars) and ocfg.warmup and (self.total_step + 1) <= ocfg.warmup_steps
            if warmup and ((self.total_step + 1) % warmup_step_rate == 0 or self.total_step == 0):
                ratio = (self.total_step + 1) / ocfg.warmup_steps
                for param_group in self.optimizer.param_groups:
                    param_group["lr"] = ratio * param_group["initial_lr"]
                lrs = " ".join(f"{g['lr']:.2e}" for g in self.optimizer.param_groups)
                self.echo(f"warmup lr: {lrs} @ {self.total_step}")
            loss = self.step(*inputs)
            if not ocfg.use_lars and ocfg.batch_sch and not warmup:
                self.scheduler.step()               # after all warm-up is completed (cvalp.py:207-209)
            self.timeit(all_time, key="model")
            self.total_step += 1
            self.total_loss += loss.detach()
            self.total_inst += ninst * nchunk
            if self.cfg.rank <= 0 and self.total_step % self.cfg.running.peep_rate == 0:
                lr_w = self.optimizer.param_groups[0]["lr"]
                lr_b = self.optimizer.param_groups[1]["lr"]
                msg = self.model.report(**{"nstep": self.total_step})
                self.echo(
                    f"epoch {iepoch:>4} step {self.total_step}\t"
                    f"lr_w {lr_w:.2e} lr_b {lr_b:.2e} loss {float(self.total_loss) / self.total_step:.3f} "
                    f"{msg} {self.total_inst / (time.time() - self.start_time):.2f} samples/s"
                )
            if self.total_step % self.cfg.running.save_rate == 0 or (
                    self.cfg.running.save_epoch and self.total_step % len(self.dataloader) == 0):
                for loader, samples in ((self.evalloader, self.cfg.running.eval_samples),
                                        (self.testloader, self.cfg.running.test_samples)):
                    if loader is None:
                        continue
                    self.model.train(False)
                    with torch.no_grad():
                        report = self.infer(loader, samples=samples, iepoch=iepoch, gold_file=self.gold_file)
                    self.model.train(True)
                    if report != "":
                        self.echo(f"{report}")
                if self.cfg.rank <= 0:
                    self.save()
            self.timeit(all_time, key="report")
        if not ocfg.use_lars and not ocfg.batch_sch:
            self.scheduler.step()                   # per-epoch schedule (cvalp.py:270-271)
        self.timeit(all_time, show=True)

    # ------------------------------------------------------------------ cvalp.py:274-300
    def infer(self, dataloader, samples=float("inf"), iepoch=0, gold_file=None):
        nsample, nchunk = 0, 1
        start_time = time.time()
        for ibatch, batch in enumerate(dataloader):
            if nsample >= samples:
                break
            images, audios, text, _, names = self.make_batch(batch)
            self.model(images, audios, text if self.with_text else None, names=names)
            nsample += images.shape[0] * nchunk
        self.echo(f"# sample {nsample}; {nsample / (time.time() - start_time):.2f} samples/s")
        return self.model.report(gold_file=gold_file)

    # ------------------------------------------------------------------ cvalp.py:302-309
    def save(self):
        from .config import to_plain
        out_dir = f"{self.cfg.alias_root}/{self.cfg.model_name}"
        os.makedirs(out_dir, exist_ok=True)
        fsave = f"{out_dir}/{self.total_step:08d}.pth"
        self.echo(f"Saving the checkpoint to {fsave}")
        torch.save({"cfg": to_plain(self.cfg), "model": self.model.collect_audio_state_dict()}, fsave)

    # ------------------------------------------------------------------ cvalp.py:311-348
    def build_optimizer(self, tunable_params={}):
        if not self.model.training:
            return
        self.params = list(tunable_params.values())
        for k, v in self.model.named_parameters():
            if k not in tunable_params:
                v.requires_grad = False
        ntotal = sum(p.numel() for p in self.model.parameters())
        ntune = sum(p.numel() for p in self.model.parameters() if p.requires_grad)
        self.echo(f"# param {ntotal / 1e6:.2f}M # tunable {ntune / 1e6:.2f}M.")
        # transformer-stack parameters are reduced per layer by the backward itself (parallel.GradSync)
        for head in (self.model.audio_head, getattr(self.model, "image_head", None), getattr(self.model, "text_head", None)):
            if head is not None and hasattr(head, "encoder"):
                for p in head.encoder.parameters():
                    p._vipant_bucketed = True
        param_groups = [
            {"params": [p for p in self.params if p.ndim > 1]},
            {"params": [p for p in self.params if p.ndim < 2]},
        ]
        ocfg = self.cfg.optimizer
        if ocfg.use_lars:
            self.optimizer = LARS(param_groups, lr=0., weight_decay=ocfg.weight_decay,
                                  weight_decay_filter=exclude_bias_or_norm, lars_adaptation_filter=exclude_bias_or_norm)
            # `running.batch_size` is PER PROCESS here (one process per GPU), while the reference's dp mode feeds every GPU from
            # one process: say which global batch and base learning rate this launch trains with (module/lars.py)
            world = parallel.world_size()
            self.echo(f"LARS schedule: per-process batch {ocfg.batch_size} x {world} replica(s) = global batch "
                      f"{ocfg.batch_size * world}, base lr {ocfg.batch_size * world / 256:g}")
        else:
            # cvalp.py:338-342: any torch.optim optimizer + lr scheduler named in the config (`optimizer.optimizer`,
            # `optimizer.scheduler`).  The update itself runs through torch's own optimizer kernels -- only LARS, the default
            # of both launch scripts, has a fused HIP step; forward / backward are the HIP path either way.
            ocfg_opt, ocfg_sch = ocfg.optimizer, ocfg.scheduler
            self.optimizer = getattr(torch.optim, ocfg_opt[0])(param_groups, **dict(ocfg_opt[1]))
            self.scheduler = getattr(torch.optim.lr_scheduler, ocfg_sch[0])(self.optimizer, **dict(ocfg_sch[1]))
        if self.cfg.verbose:
            self.echo("Gradienting The Following Parameters:")
            for k, v in self.model.named_parameters():
                if v.requires_grad:
                    self.echo(f"{k} {tuple(v.size())}")


class VALMonitor(Monitor):
    """AT fine-tuning trainer (cvap/monitor/cvalp.py:23)."""
    with_text = True


class VAMonitor(Monitor):
    """VA pre-training trainer (cvap/monitor/cvap.py:21)."""
    with_text = False


class VASMonitor(Monitor):
    """Siamese multi-view VA trainer (cvap/monitor/siamese_va.py:19-180; `monitor=VASMonitor worker=CVASP +running=siamese`).  The
    epoch loop is the base trainer's; what differs is the batch -- five slots, of which only the views that a live pair of
    `model.loss` reads are moved to the device, image views rescaled bilinearly to `running.resolution` -- and the worker's
    signature.  View slots that hold uint8 frames (`running.image_frames`) become the prime and the second `barlow` view of
    vipant_amd/image_views.py instead (`clip` under `running.clip_tf` and at evaluation); the second only when `model.loss.vv`.
    With `running.data_root` the batch comes from the siamese raw-file dataset (vipant_amd/data: frames and PCM once, `SecondView`
    markers in the second view slots) and both audio views from one log-mel launch (`audio_views_from_pcm`)."""
    with_text = False
    # FbankTransform's own normalisation (cvap/data/audio/transform.py:228-229, :238-239, :247-248): the siamese dataset does not
    # read `running.audio.norms`
    FBANK_NORMS = (-4.93839311, 5.75751113)
    PRIME_MASKS = (32, 200)         # transform_prime: FrequencyMasking(32), TimeMasking(200) -> view 1
    SECOND_MASKS = (48, 300)        # transform: FrequencyMasking(48), TimeMasking(300) -> view 2

    def eval_norms(self):
        raise VipantError("running.audio.eval_norms under running.multi_view: the siamese dataset normalises with FbankTransform's "
                          "own constants and has no statistics run (take them with monitor=VAMonitor)")

    def siamese_frontend(self, train, sample_rate):
        from .frontend import KaldiFbank
        cache = self.__dict__.setdefault("_siamese_fbank", {})
        key = (bool(train), int(sample_rate))
        if key not in cache:
            acfg = self.cfg.running.audio
            cache[key] = KaldiFbank(float(sample_rate), acfg.num_mel_bins, acfg.max_len, self.FBANK_NORMS, acfg.get("zero_mean_wf", True),
                                    acfg.get("frame_shift", 10), device=self.device, train=train)
        return cache[key]

    def audio_views_from_pcm(self, clips):
        """A PcmBatch -> (view 1, view 2 or None), log-mels [b, 1, T, F] on the device, as the siamese dataset makes them
        (cvap/data/image_audio.py:256-285, transform.py:223-258): H2D, the waveform (`pcm_wave`, channel 0, no tiling), then ONE
        log-mel launch that writes both views (`vipant_fbank_view_pair`).  No waveform chain whatever `running.audio.transform_audio`
        says (:238); the pipeline's crop of a clip longer than `crop_len`, drawn when training and centred at evaluation;
        `zero_mean_wf` from the config; FbankTransform's constants, not `running.audio.norms`.  Training masks view 1 with the prime
        set (32, 200) and view 2 with the second set (48, 300); view 2 exists only under `model.loss.aa` (otherwise the single
        `vipant_fbank_view` launch).  Evaluation: view 1 unmasked, no view 2.
        Draws per training step, from the per-rank generator `_aug_generator()` in this order: `draw_views(b)` if a clip of the
        batch is longer than `crop_len`; `draw_masks(b, freq_mask_param=32, time_mask_param=200)`; under `model.loss.aa`
        `draw_masks(b, freq_mask_param=48, time_mask_param=300)`.  Evaluation draws nothing."""
        from .frontend import pcm_wave
        train, both = self._training(), bool(self.cfg.model.loss.aa)
        fbank = self.siamese_frontend(train, clips.sample_rate)
        n = torch.minimum(clips.nframes, clips.pcm.shape[1] // clips.channels.clamp(1, 8).long()).clamp_(min=0)      # (no device sync)
        longest = int(n.max())
        on_dev = clips.to(self.device, non_blocking=True)
        wave, nsamples = pcm_wave(on_dev.pcm, on_dev.nframes, on_dev.channels, mode="first", wave_stride=max(8, -(-longest // 8) * 8))
        b = wave.shape[0]
        if not train:
            return fbank(wave, nsamples, view=True), None
        if "aug_generator" not in self.__dict__:
            self.aug_generator = self._aug_generator()
        view = fbank.draw_views(b, self.aug_generator) if longest > fbank.crop_len else fbank.no_views(b)
        masks = fbank.draw_masks(b, self.aug_generator, freq_mask_param=self.PRIME_MASKS[0], time_mask_param=self.PRIME_MASKS[1])
        if not both:
            return fbank(wave, nsamples, masks=masks, view=view), None
        masks2 = fbank.draw_masks(b, self.aug_generator, freq_mask_param=self.SECOND_MASKS[0], time_mask_param=self.SECOND_MASKS[1])
        return fbank(wave, nsamples, masks=masks, view=view, masks2=masks2, pair=True)

    def make_batch(self, batch):
        """The six slots of a siamese batch -> tensors on the device.  A file batch (`running.data_root`) holds a FrameBatch and a
        PcmBatch in the first view slots and SecondView markers in the second: one upload of the frames serves both image views,
        one upload of the PCM both audio views (`audio_views_from_pcm`)."""
        lcfg, res = self.cfg.model.loss, self.cfg.running.resolution

        def to_dev(x):
            return torch.as_tensor(x).to(self.device, non_blocking=True)

        def scale_images(images):
            if images.dim() != 2 and images.shape[-1] != res and list(images.shape[1:]) != [1, 1, 1]:
                images = torch.nn.functional.interpolate(images, res, mode="bilinear", align_corners=False)
            return images
        images = to_dev(batch[0]) if lcfg.vp or lcfg.ap else None
        if isinstance(batch[1], FrameBatch):
            second = batch[batch[2].of] if isinstance(batch[2], SecondView) else batch[2]
            if second is not batch[1]:
                raise VipantError("a siamese file batch: the second image view must be a view of the first slot's frames")
            frames, hw = batch[1].frames.to(self.device, non_blocking=True), batch[1].hw
            images_v1 = scale_images(self.image_views(frames, "prime", siamese=True, hw=hw))
            images_v2 = scale_images(self.image_views(frames, "second", siamese=True, hw=hw)) if lcfg.vv else None
        else:
            images_v1 = scale_images(self.image_views(to_dev(batch[1]), "prime", siamese=True))
            images_v2 = scale_images(self.image_views(to_dev(batch[2]), "second", siamese=True)) if lcfg.vv else None
        if isinstance(batch[3], PcmBatch):
            second = batch[batch[4].of] if isinstance(batch[4], SecondView) else batch[4]
            if second is not batch[3]:
                raise VipantError("a siamese file batch: the second audio view must be a view of the first slot's clips")
            audios_v1, audios_v2 = self.audio_views_from_pcm(batch[3])
        else:
            audios_v1 = to_dev(batch[3]).unsqueeze(1)
            audios_v2 = to_dev(batch[4]).unsqueeze(1) if lcfg.aa else None
        return images, images_v1, images_v2, audios_v1, audios_v2, batch[-1]

    def _step_inputs(self, batch):
        images, images_v1, images_v2, audios_v1, audios_v2, _ = batch
        return (images, images_v1, images_v2, audios_v1, audios_v2), (images if images is not None else audios_v1).shape[0]

    def step(self, images, images_v1, images_v2, audios_v1, audios_v2):
        self.optimizer.zero_grad(set_to_none=True)
        loss = self.model(images, images_v1, audios_v1, text_v1=None, images_v2=images_v2, audios_v2=audios_v2)
        self._backward(loss)
        self._reduce_and_update()
        return loss

    def infer(self, dataloader, samples=float("inf"), iepoch=0, gold_file=None):
        nsample = 0
        start_time = time.time()
        for ibatch, batch in enumerate(dataloader):
            if nsample >= samples:
                break
            images, images_v1, _, audios_v1, _, names = self.make_batch(batch)
            self.model(images, images_v1, audios_v1, names=names)
            nsample += (images if images is not None else audios_v1).shape[0]
        self.echo(f"# sample {nsample}; {nsample / (time.time() - start_time):.2f} samples/s")
        return self.model.report(gold_file=gold_file)


class SyntheticFolds:
    """Labelled x-fold data with the contract of the reference's ESC-50 / UrbanSound8K collator (cvap/data/esc50.py): batches of
    (audios [b, T, F] fp32, labels int64 [b], names).  Dataset-free and seeded: sample i of a fold has class i mod C and the
    spectrogram `prototype[class] + noise`, so the classes are separable and a classifier can be seen to learn.  `loader_list`
    holds, per fold, (train loader factory over the other folds -- reshuffled every epoch --, eval loader factory over the fold
    held out), as `build_xfold_dataloader_list` returns them; under replicas a rank takes every world-th training batch."""

    class _Loader:
        def __init__(self, owner, folds, batch, shuffle, shard):
            self.owner, self.folds, self.b, self.shuffle, self.shard = owner, list(folds), int(batch), shuffle, shard
            self.index = [(f, i) for f in self.folds for i in range(owner.per_fold)]
            self.epoch = 0
            nb = len(self.index) // self.b if shuffle else -(-len(self.index) // self.b)
            self.nbatch = nb // shard[1] if shard[1] > 1 else nb

        def __len__(self):
            return self.nbatch

        def __iter__(self):
            order = list(range(len(self.index)))
            if self.shuffle:
                g = torch.Generator().manual_seed(self.owner.seed + 7919 * self.epoch + 31 * sum(self.folds))
                order = torch.randperm(len(order), generator=g).tolist()
                self.epoch += 1
            rank, world = self.shard
            for ib in range(self.nbatch):
                k = ib * world + rank if world > 1 else ib
                picks = [self.index[j] for j in order[k * self.b:(k + 1) * self.b]]
                yield self.owner.batch(picks)

    def __init__(self, cfg, nfold, nclass, per_fold, shard=(0, 1)):
        rcfg = cfg.running
        self.seed, self.nfold, self.nclass, self.per_fold = int(cfg.seed), int(nfold), int(nclass), int(per_fold)
        self.T, self.F = int(rcfg.max_audio_len), int(rcfg.num_mel_bins)
        g = torch.Generator().manual_seed(self.seed)
        self.proto = torch.randn(self.nclass, self.T, self.F, generator=g)
        b = int(rcfg.batch_size)
        every = list(range(self.nfold))
        self.loader_list = [
            ((lambda k=k: (None, self._Loader(self, [f for f in every if f != k] or [k], b, True, shard))),
             (lambda k=k: (None, self._Loader(self, [k], b, False, (0, 1)))))
            for k in every]
        self.lid2str = [f"class {c}" for c in range(self.nclass)]
        self.lid2int = _synthetic_prompts(self.seed + 1, self.nclass)
        self.label_map = None

    def batch(self, picks):
        labels = torch.tensor([i % self.nclass for _, i in picks], dtype=torch.int64)
        audios = torch.empty(len(picks), self.T, self.F)
        for n, (f, i) in enumerate(picks):
            g = torch.Generator().manual_seed(self.seed + 100003 * (f + 1) + i)
            audios[n] = self.proto[i % self.nclass] + torch.randn(self.T, self.F, generator=g)
        return audios, labels, [f"synthetic-fold{f}-{i}" for f, i in picks]


class ESCMonitor(Monitor):
    """x-fold supervised classification trainer (cvap/monitor/esc50_clf.py:24-386; `monitor=ESCMonitor`, `running=esc50` /
    `us8k`): per fold a fresh model is trained for `optimizer.epochs` epochs and evaluated on the held-out fold after every
    epoch; `summary_report` prints the best-epoch and per-fold-maximum precision statistics.  `eval=True running.zero_shot=True`
    classifies every fold by the text tower's prompt features instead.  AMP's GradScaler (esc50_clf.py:88, 179-183) has no
    counterpart: bf16 operands with fp32 accumulation and fp32 master weights need no loss scaling."""

    def __init__(self, cfg, echo, device, loader_list=None):
        self.cfg, self.echo, self.device = cfg, echo, device
        self.dataloader = self.evalloader = self.testloader = None
        self.gold_file = None
        output_dim = self.build_data(loader_list)
        self._build_model(output_dim)

    def _build_model(self, output_dim):
        model = build_main_model(self.cfg, self.echo)
        tunable_params = model.build(output_dim=output_dim)
        self.model = model
        self._configure(model)
        self.model.train(not self.cfg.eval)
        self.build_optimizer(tunable_params)

    def reinitialize(self, cfg, echo):
        self.echo("Reinitialize everything except `dataloader_list`.")
        self._build_model(len(self.lid2str))

    def build_data(self, loader_list=None):
        rcfg = self.cfg.running
        if loader_list is not None:
            self.loader_list, self.lid2str, self.lid2int, self.label_map = loader_list
            return len(self.lid2str)
        if self._from_files():                                    # esc50_clf.py:41-49: ESC-50 / UrbanSound8K from `running.data_root`
            from .data import build_xfold_dataloader_list
            self.loader_list, self.lid2str, self.lid2int, self.label_map = build_xfold_dataloader_list(self.cfg, echo=self.echo)
            self.echo(f"Instantiate {len(self.loader_list)}-fold dataloaders from `{rcfg.data_name}': {len(self.lid2str)} classes.")
            return len(self.lid2str)
        shard = (parallel.rank(), parallel.world_size()) if parallel.active() else (0, 1)
        data = SyntheticFolds(self.cfg, rcfg.get("synthetic_folds", 2), rcfg.get("synthetic_classes", 50),
                              int(rcfg.get("synthetic_steps", 8)) * int(rcfg.batch_size), shard)
        self.loader_list, self.lid2str, self.lid2int, self.label_map = data.loader_list, data.lid2str, data.lid2int, data.label_map
        self.echo(f"Instantiate {len(self.loader_list)}-fold dataloaders from `synthetic': {data.per_fold} samples per fold, "
                  f"{len(self.lid2str)} classes.")
        return len(self.lid2str)

    # ------------------------------------------------------------------ esc50_clf.py:58-102
    def learn(self):
        if not self.model.training:
            if self.cfg.running.get("zero_shot", False):
                self.echo("(Zero-shot) Evaluating started...")
                with torch.no_grad():
                    report = self.standard_zero_shot()
                self.echo(f"{report}")
                return None
            self.echo("Evaluating started...")
            with torch.no_grad():
                for ifold, (_, evalloader_fn) in enumerate(self.loader_list):
                    report = self.infer(evalloader_fn()[1], samples=self.cfg.running.eval_samples)
                    self.echo(f"{ifold:>2}th fold: {report}")
            return None
        report_by_fold = []
        for ifold, (dataloader_fn, evalloader_fn) in enumerate(self.loader_list):
            _, self.dataloader = dataloader_fn()
            _, self.evalloader = evalloader_fn()
            self.echo(f"Training started ({ifold})...")
            self.last_time = 0.
            self.total_loss = 0
            self.total_step = 0
            self.total_inst = 0
            self.start_time = time.time()
            self.report_by_epoch = []
            for iepoch in range(int(self.cfg.optimizer.epochs)):
                self.epoch(iepoch)
            report_by_fold.append(self.report_by_epoch)
            self.reinitialize(self.cfg, self.echo)
        self.report_by_fold = report_by_fold
        self.summary_report(report_by_fold)

    # ------------------------------------------------------------------ esc50_clf.py:104-120
    def summary_report(self, report):
        report = np.array(report)
        if report.ndim < 2 or report.shape[1] == 0:       # a rank other than 0 gets no report string: nothing to summarise
            return
        self.echo(f"\n{report}")
        nfold, nepoch = report.shape[:2]
        self.echo(f"Total {nepoch} epochs for each of {nfold} folds.")
        report_sum = report.sum(0)
        best_epoch = report_sum.argmax()
        best_precisions = report[:, best_epoch]
        mean, std = best_precisions.mean(), best_precisions.std()
        self.echo(f"Best mean and std: {mean:2.2f} \\pm {std:2.2f} in the {best_epoch}th epoch.")
        max_epoch = report.argmax(1)
        max_precisions = report.max(1)
        mean, std = max_precisions.mean(), max_precisions.std()
        self.echo(f"Max mean and std: {mean:2.2f} \\pm {std:2.2f} in the {max_epoch}th epoch.")

    # ------------------------------------------------------------------ esc50_clf.py:122-132
    def make_batch(self, batch):
        if isinstance(batch[0], PcmBatch):                          # decoded clips of a file dataset: never tiled (esc50.py:81)
            audios = self.audios_from_pcm(batch[0], tile=False)
        else:
            audios = torch.as_tensor(batch[0]).to(self.device, non_blocking=True).unsqueeze(1)
        labels = torch.as_tensor(batch[1]).to(self.device, non_blocking=True)
        return audios, labels, batch[2]

    def step(self, audios, labels):
        """zero_grad -> forward -> backward -> (replica gradient reduction) -> optimizer (esc50_clf.py:178-183).  Unlike the
        contrastive heads' gradients, a classification head's are partial per rank (every rank scores its own rows, scaled by
        1 / world): they join the SUM all-reduce with the other parameters outside the per-block buckets."""
        from . import ops
        self.optimizer.zero_grad(set_to_none=True)
        loss = self.model(audios, labels)
        loss.backward(gradient=ops.unit_grad(loss.device) if loss.is_cuda and loss.dim() == 0 and loss.dtype == torch.float32 else None)
        if self.grad_sync is not None:
            self.grad_sync.reduce_params([p for p in self.params if not getattr(p, "_vipant_bucketed", False)])
            self.grad_sync.wait()
        self.optimizer.step()
        return loss

    # ------------------------------------------------------------------ esc50_clf.py:150-238
    def epoch(self, iepoch):
        import re
        all_time = defaultdict(list)
        self.timeit(all_time)
        nchunk = parallel.world_size()
        ocfg = self.cfg.optimizer
        warmup_step_rate = max(int(ocfg.warmup_steps) // 20, 1)
        for step, batch in enumerate(self.dataloader, start=iepoch * len(self.dataloader)):
            audios, labels, _ = self.make_batch(batch)
            self.timeit(all_time, key="data")
            if ocfg.use_lars:
                adjust_learning_rate(ocfg, self.optimizer, self.dataloader, step)
            warmup = (not ocfg.use_lars) and ocfg.warmup and self.total_step <= ocfg.warmup_steps
            if warmup and (self.total_step % warmup_step_rate == 0 or self.total_step == 0):
                ratio = self.total_step / ocfg.warmup_steps
                for param_group in self.optimizer.param_groups:
                    param_group["lr"] = ratio * param_group["initial_lr"]
                lrs = " ".join(f"{g['lr']:.2e}" for g in self.optimizer.param_groups)
                self.echo(f"warmup lr: {lrs} @ {self.total_step}")
            loss = self.step(audios, labels)
            if not ocfg.use_lars and ocfg.batch_sch and not warmup:
                self.scheduler.step()
            self.timeit(all_time, key="model")
            self.total_step += 1
            self.total_loss += loss.detach()
            self.total_inst += audios.shape[0] * nchunk
            if self.cfg.rank <= 0 and self.total_step % self.cfg.running.peep_rate == 0:
                lr_w = self.optimizer.param_groups[0]["lr"]
                lr_b = self.optimizer.param_groups[1]["lr"]
                self.echo(
                    f"epoch {iepoch:>4} step {self.total_step}\t"
                    f"lr_w {lr_w:.2e} lr_b {lr_b:.2e} loss {float(self.total_loss) / self.total_step:.3f} "
                    f"{self.total_inst / (time.time() - self.start_time):.2f} samples/s"
                )
            if self.total_step % self.cfg.running.save_rate == 0 or (
                    self.cfg.running.save_epoch and self.total_step % len(self.dataloader) == 0):
                report = ""
                if self.evalloader is not None:
                    self.model.train(False)
                    with torch.no_grad():
                        report = self.infer(self.evalloader, samples=self.cfg.running.eval_samples, iepoch=iepoch)
                    self.model.train(True)
                if report != "":
                    precision = re.search(r"=\s(\d+\.\d+)\s\@", report)
                    assert precision is not None, f"invalid report: `{report}`"
                    self.report_by_epoch.append(float(precision.group(1)))
                    self.echo(f"{report}")
            self.timeit(all_time, key="report")
        if not ocfg.use_lars and not ocfg.batch_sch:
            self.scheduler.step()
        self.timeit(all_time, show=True)

    # ------------------------------------------------------------------ esc50_clf.py:240-258
    def infer(self, dataloader, samples=float("inf"), iepoch=0, gold_file=None):
        nsample = 0
        start_time = time.time()
        for ibatch, batch in enumerate(dataloader):
            if nsample >= samples:
                break
            audios, labels, names = self.make_batch(batch)
            self.model(audios, labels, names=names)
            nsample += audios.shape[0]
        self.echo(f"# sample {nsample}; {nsample / (time.time() - start_time):.2f} samples/s")
        return self.model.report()

    # ------------------------------------------------------------------ esc50_clf.py:294-325
    def standard_zero_shot(self, samples=float("inf"), iepoch=0):
        import re
        text_features = self.model.encode_text(torch.tensor(self.lid2int, device=self.device))
        for ifold, (_, evalloader_fn) in enumerate(self.loader_list):
            _, dataloader = evalloader_fn()
            nsample = 0
            start_time = time.time()
            for ibatch, batch in enumerate(dataloader):
                if nsample >= samples:
                    break
                audios, labels, names = self.make_batch(batch)
                self.model(audios, labels, names=names)
                nsample += audios.shape[0]
            self.echo(f"{ifold:>2}th fold: # sample {nsample}; {nsample / (time.time() - start_time):.2f} samples/s")
        report = self.model.report(text=text_features, label_map=self.label_map)
        self.echo(f"{report}")
        precision = re.search(r"=\s(\d+\.\d+)\s\@", report)
        assert precision is not None, f"invalid report: `{report}`"
        return f"{float(precision.group(1)):2.2f} for zero-shot classification."


class SyntheticTagging:
    """Seeded multi-label batches with the contract of the reference's AudioSet collator (cvap/data/audioset_cls.py):
    (images, audios, text, multi-hot labels [b, C], names) with dummy [b, 1, 1, 1] images.  A clip has 1-3 positive classes and is
    the sum of their prototypes plus noise.  `running.synthetic_wave=True`: the audio slot holds WAVEFORMS fp32 [b, n] -- a class
    is a tone of its own frequency -- and the text slot their valid lengths int64 [b]; the trainer runs the GPU front-end on them
    (waveform mixup needs the waveform).  False: spectrograms [b, T, F] as the reference collator yields them (a class is a
    pattern over the mel bins).  Under replicas a rank draws its own batches."""

    def __init__(self, cfg, steps, train, rank=0):
        rcfg = cfg.running
        self.steps, self.train, self.rank = int(steps), bool(train), int(rank)
        self.b, self.nclass = int(rcfg.batch_size), int(rcfg.get("synthetic_classes", 527))
        self.wave = bool(rcfg.get("synthetic_wave", True))
        self.sr = float(rcfg.get("sample_rate", 16000))
        self.n = int(self.sr * float(rcfg.get("synthetic_seconds", 10.0)))
        self.T, self.F = int(rcfg.max_audio_len), int(rcfg.num_mel_bins)
        self.seed = int(cfg.seed) + (0 if train else 500009)
        g = torch.Generator().manual_seed(int(cfg.seed) + 2)
        self.freq = 100.0 + (0.45 * self.sr - 100.0) * torch.rand(self.nclass, generator=g)      # Hz, below Nyquist
        self.proto = torch.randn(self.nclass, self.F, generator=g)
        self.lid2int = _synthetic_prompts(int(cfg.seed) + 1, self.nclass)

    def __len__(self):
        return self.steps

    def __iter__(self):
        for step in range(self.steps):
            g = torch.Generator().manual_seed(self.seed + 1000 * self.rank + step)
            labels = torch.zeros(self.b, self.nclass, dtype=torch.int64)
            npos = torch.randint(1, 4, (self.b,), generator=g)
            for i in range(self.b):
                labels[i, torch.randperm(self.nclass, generator=g)[:int(npos[i])]] = 1
            y = labels.float()
            if self.wave:
                t = torch.arange(self.n, dtype=torch.float32) / self.sr
                phase = 2.0 * np.pi * torch.rand(self.b, self.nclass, generator=g)
                audios = torch.zeros(self.b, self.n)
                for i in range(self.b):
                    for c in labels[i].nonzero().flatten().tolist():
                        audios[i] += 0.1 * torch.sin(2.0 * np.pi * float(self.freq[c]) * t + float(phase[i, c]))
                audios += 0.01 * torch.randn(self.b, self.n, generator=g)
                text = torch.full((self.b,), self.n, dtype=torch.int64)
            else:
                audios = (y @ self.proto).unsqueeze(1) + torch.randn(self.b, self.T, self.F, generator=g)
                text = torch.zeros(self.b, 1, dtype=torch.int64)
            names = [f"synthetic-{'train' if self.train else 'eval'}-{self.rank}-{step}-{i}" for i in range(self.b)]
            yield torch.zeros(self.b, 1, 1, 1), audios, text, labels, names


class ASMonitor(Monitor):
    """AudioSet tagging trainer (cvap/monitor/audioset_clf.py:25-467 without `eval_norms` and `repeated_zero_shot`;
    `monitor=ASMonitor worker=ASClassifier +running=audioset +model/loss=bce`).  The epoch loop, schedules, peep line, periodic
    eval and checkpoint are the base trainer's.  What differs is the batch: waveform batches go through the GPU front-end
    (vipant_amd/frontend.py) inside `make_batch`, and when training with `running.mixup_rate > 0` the clips are mixed in the
    front-end's launch and the labels become lam y + (1 - lam) y[partner], which BCELossHead scores as fractions
    (`soft_targets`).  With `running.data_root=DIR` the batches come from the raw-file tagging dataset (vipant_amd/data/classify.py):
    as in the reference a loader worker draws a clip's partner from the whole DATASET, the partner clips ride behind the batch,
    the launch reads them as rows that produce no output (`KaldiFbank(mix=, outputs=)`, vipant_fbank_mix_src) and the soft
    targets are formed on the device from the ragged class lists (vipant_multihot_mix).  Synthetic batches (`data_root` empty)
    keep the in-batch rule: the trainer draws the partner among the clips of the batch (`draw_mixup`).  Without mixup
    (`running.clf=False`, or `mixup_rate` 0) the batch takes the reference's other branch: the `running.audio.audio_transforms`
    chain when `transform_audio` is on and the model is training, and the crop rule for clips longer than the front-end's
    `crop_len`, both inside the front-end's launch (`KaldiFbank.draw_views`, `view=`).
    `eval=True running.zero_shot=True` scores the clips against one prompt per class through the text tower."""
    with_text = False
    partial_head_grads = True

    def __init__(self, cfg, echo, device, dataloader=None):
        self.cfg, self.echo, self.device = cfg, echo, device
        self.evalloader = self.testloader = None
        self.gold_file = None
        self.mixup_rate = float(cfg.running.get("mixup_rate", 0.0) or 0.0)
        self.aug_generator = self._aug_generator()
        self._fbank = {}
        output_dim = self.build_data(dataloader)
        model = build_main_model(cfg, echo)
        tunable_params = model.build(output_dim=output_dim)
        self.model = model
        self._configure(model)
        self.model.train(not cfg.eval)
        self.model.loss_head.soft_targets = self.mixup_rate > 0
        self.build_optimizer(tunable_params)

    def _aug_generator(self):
        """The host generator of the mixup and SpecAugment draws: seeded per rank, consumed in step order."""
        return torch.Generator().manual_seed(int(self.cfg.seed) + 7 + 1000 * max(int(self.cfg.rank), 0))

    def build_data(self, dataloader=None):
        rcfg = self.cfg.running
        if dataloader is None and self._from_files():
            return self.build_file_data()
        steps, rank = int(rcfg.get("synthetic_steps", 8)), max(int(self.cfg.rank), 0)
        evalloader = SyntheticTagging(self.cfg, steps, False, 0)
        self.lid2int = evalloader.lid2int
        if self.cfg.eval:
            self.dataloader = dataloader if dataloader is not None else evalloader
        else:
            self.dataloader = dataloader if dataloader is not None else SyntheticTagging(self.cfg, steps, True, rank)
            self.evalloader = evalloader if rcfg.eval_name else None
        self.echo(f"Instantiate main dataloader from `synthetic': total {len(self.dataloader)} batches, "
                  f"{evalloader.nclass} sound classes.")
        return evalloader.nclass

    # ------------------------------------------------------------------ audioset_clf.py:100-145
    def build_file_data(self):
        """`running.data_root=DIR`: label map and filter set, the main loader (`eval_name` when evaluating) and, when training, the
        evaluation and test loaders whose index exists; `lid2int` = the label map's prompts, one ragged token row per class."""
        from .data import build_audioset_clf_dataloader, build_audioset_label_map, build_filter_set
        rcfg = self.cfg.running
        label_map = build_audioset_label_map(rcfg.data_root, label_map=rcfg.label_map, prompt=str(rcfg.get("prompt", "") or ""), rcfg=rcfg)
        lid2int = [0] * len(label_map)
        for k, v in label_map.items():
            lid2int[v[0]] = v[2]
        self.lid2int = lid2int
        filters = build_filter_set(rcfg.data_root, rcfg.get("filter_set", None))
        if filters is not None:
            self.echo(f"At most {len(filters)} audio clips for training becuase of filtering.")
        self.echo(f"Total {len(label_map)} sound classes.")
        data_name = rcfg.eval_name if self.cfg.eval else rcfg.data_name
        _, self.dataloader = build_audioset_clf_dataloader(
            self.cfg, data_name, label_map, shuffle=(not self.cfg.eval and not rcfg.audio.get("eval_norms", False)),
            train=(not self.cfg.eval), filters=filters, echo=self.echo)
        self.echo(f"Instantiate main dataloader from `{data_name}': total {len(self.dataloader)} batches.")
        self.gold_file = f"{rcfg.data_root}/{data_name}.csv"

        def side_loader(name):
            name = "IGNORE_ME" if self.cfg.eval else str(name or "IGNORE_ME")
            path = f"{rcfg.data_root}/{name}"
            if not (os.path.isdir(path) or os.path.isfile(f"{path}.csv")):
                return None
            return build_audioset_clf_dataloader(self.cfg, name, label_map, shuffle=False, train=False, echo=self.echo)[1]
        self.evalloader = side_loader(rcfg.eval_name)
        if self.evalloader is not None:
            self.echo(f"Will do evaluation every {rcfg.save_rate} steps on {len(self.evalloader)} batches ({rcfg.eval_name}).")
            self.gold_file = f"{rcfg.data_root}/{rcfg.eval_name}.csv"
        self.testloader = side_loader(rcfg.test_name)
        if self.testloader is not None:
            self.echo(f"Will do test every {rcfg.save_rate} steps on {len(self.testloader)} batches ({rcfg.test_name}).")
            self.gold_file_test = f"{rcfg.data_root}/{rcfg.test_name}.csv"
        return len(label_map)

    def frontend(self, train):
        from .frontend import KaldiFbank
        if train not in self._fbank:
            self._fbank[train] = KaldiFbank.from_config(self.cfg.running.audio, float(self.cfg.running.get("sample_rate", 16000)),
                                                        train=train, device=self.device)
        return self._fbank[train]

    @staticmethod
    def soft_labels(labels, index, lam):
        """lam y + (1 - lam) y[partner] (audioset_cls.py:400); a clip without a partner (index -1, lam 1) keeps its labels exactly."""
        y = labels.float()
        index = index.to(y.device).long()
        lam = lam.to(y.device).unsqueeze(1)
        partner = torch.where(index < 0, torch.arange(y.shape[0], device=y.device), index)
        return lam * y + (1.0 - lam) * y[partner]

    def make_tagging_batch(self, batch):
        """A batch of the raw-file tagging dataset (TaggingCollator): b clips and, behind them, the p partner clips the workers drew
        (audioset_cls.py:374-400).  H2D and the waveform of all b + p rows (`pcm_wave`: channel 0, never tiled -- `wf[:1]`), masks
        for the b outputs, then one log-mel launch that mixes on the way into LDS and writes b rows, and one launch that forms
        the (soft) multi-hot targets from the ragged class lists.  The waveform is always zero-mean (:377), a longer clip is cut at
        `max_len` frames (:410).  At evaluation there are no partners and no masks, and the targets are exact {0, 1}."""
        from . import ops
        from .frontend import pcm_wave
        clips, tags = batch[1], batch[3]
        images = self.image_views(torch.as_tensor(batch[0]).to(self.device, non_blocking=True))
        train = self.model.training
        fbank = self.pcm_frontend(train, clips.sample_rate)
        b = int(tags.mix_index.shape[0])
        n = torch.minimum(clips.nframes, clips.pcm.shape[1] // clips.channels.clamp(1, 8).long()).clamp_(min=0)
        on_dev = clips.to(self.device, non_blocking=True)
        wave, nsamples = pcm_wave(on_dev.pcm, on_dev.nframes, on_dev.channels, mode="first", tile_len=0,
                                  wave_stride=max(8, -(-int(n.max()) // 8) * 8))
        masks = fbank.draw_masks(b, self.aug_generator) if train else None
        tags = tags.to(self.device, non_blocking=True)
        mix = (tags.mix_index, tags.mix_lambda)
        audios = fbank(wave, nsamples, masks=masks, mix=mix, outputs=b)
        labels = ops.multihot_mix(tags.ids, tags.offsets, tags.num_label, outputs=b, mix=mix)
        if not self.model.loss_head.soft_targets:
            labels = labels.long()                                  # multi-hot marks, the dtype the synthetic loader yields
        return images, audios, None, labels, batch[-1]

    # ------------------------------------------------------------------ audioset_clf.py:192-210
    def make_batch(self, batch):
        if isinstance(batch[1], PcmBatch):
            return self.make_tagging_batch(batch)
        images = self.image_views(torch.as_tensor(batch[0]).to(self.device, non_blocking=True))
        audios = torch.as_tensor(batch[1]).to(self.device, non_blocking=True)
        labels = torch.as_tensor(batch[3]).to(self.device, non_blocking=True)
        res = self.cfg.running.resolution
        if images.dim() != 2 and images.shape[-1] != res and list(images.shape[1:]) != [1, 1, 1]:
            images = torch.nn.functional.interpolate(images, res, mode="bilinear", align_corners=False)
        if audios.dim() == 2:                                       # waveforms: log-mel, mixup and masks on the device
            train = self.model.training
            fbank = self.frontend(train)
            nsamples = torch.as_tensor(batch[2]).to(self.device, non_blocking=True)
            mix = view = None
            if self.mixup_rate > 0 and self.cfg.running.get("clf", True):      # the clf loader: mixup (audioset_cls.py:374-400)
                if train:
                    mix = fbank.draw_mixup(audios.shape[0], self.mixup_rate, self.aug_generator)
                    labels = self.soft_labels(labels, *mix)
            else:                                                              # the cst loader: waveform transforms + crop rule (:402-432)
                crop = int(torch.as_tensor(batch[2]).max()) > fbank.crop_len   # (the host's copy of the lengths: no device sync)
                if train and (fbank.chain or crop):
                    view = fbank.draw_views(audios.shape[0], self.aug_generator)
                elif crop:
                    view = True                                                # evaluation: the centred window and its rule
            masks = fbank.draw_masks(audios.shape[0], self.aug_generator) if train else None
            audios = fbank(audios.float(), nsamples, masks=masks, mix=mix, view=view)
        else:
            audios = audios.unsqueeze(1)
        return images, audios, None, labels, batch[-1]

    def _step_inputs(self, batch):
        images, audios, _, labels, _ = batch
        return (images, audios, labels), audios.shape[0]

    def step(self, images, audios, labels):
        self.optimizer.zero_grad(set_to_none=True)
        loss = self.model(images, audios, labels)
        self._backward(loss)
        self._reduce_and_update()
        return loss

    # ------------------------------------------------------------------ audioset_clf.py:147-175
    def learn(self):
        if not self.model.training and self.cfg.running.get("zero_shot", False):
            self.echo("(Zero-shot) Evaluating started...")
            with torch.no_grad():
                report = self.zero_shot(self.dataloader, samples=self.cfg.running.eval_samples, gold_file=self.gold_file)
            self.echo(f"{report}")
            return None
        return super().learn()

    # ------------------------------------------------------------------ audioset_clf.py:334-404
    def infer(self, dataloader, samples=float("inf"), iepoch=0, gold_file=None, **report_kwargs):
        nsample = 0
        start_time = time.time()
        for ibatch, batch in enumerate(dataloader):
            if nsample >= samples:
                break
            images, audios, _, labels, names = self.make_batch(batch)
            self.model(images, audios, labels, names=names)
            nsample += audios.shape[0]
        self.echo(f"# sample {nsample}; {nsample / (time.time() - start_time):.2f} samples/s")
        return self.model.report(gold_file=gold_file, **report_kwargs)

    def zero_shot(self, dataloader, samples=float("inf"), iepoch=0, gold_file=None):
        def padded(rows):                                           # audioset_clf.py:366-367: zip_longest(fillvalue=0) per chunk
            width = max(len(row) for row in rows)
            return [list(row) + [0] * (width - len(row)) for row in rows]
        text = torch.cat([self.model.encode_text(torch.tensor(padded(self.lid2int[s:s + 50]), device=self.device))
                          for s in range(0, len(self.lid2int), 50)])
        return self.infer(dataloader, samples=samples, iepoch=iepoch, gold_file=gold_file, text=text)


__all__ = ["Monitor", "VAMonitor", "VALMonitor", "VASMonitor", "ESCMonitor", "ASMonitor", "SyntheticLoader", "SyntheticFolds",
           "SyntheticTagging"]
